// CPU build of d3ga_amd/csrc/cage_author_math.h: the argument rules and the per-element text of cage_author.hip, walked in the
// kernels' order of stages.  Same arguments as the d3ga_cage_* entry points (include/d3ga.h) without the stream, host memory.
// Built by tests/cage_author_ref.py with -ffp-contract=off.
#include "../../d3ga_amd/csrc/cage_author_math.h"

using namespace d3ga;

extern "C" {

int hc_cage_voxelize(const d3ga_voxel_grid *g, int32_t V, int32_t F, const double *verts, const int32_t *faces, uint32_t *status) {
    const int st = ca_check_voxelize(g, V, F, verts, faces, status);
    if (st != 0) return st;
    for (int64_t i = 0; i < (int64_t)g->D * g->D * g->W; ++i) g->bits[i] = 0;
    for (int32_t f = 0; f < F; ++f) {
        const CaTriBox b = ca_tri_prepare(g->radius, V, verts, faces + 3 * (size_t)f);
        if (b.bad) { *status |= D3GA_CAGE_STATUS_RANGE; continue; }
        for (int64_t i = 0; i < (int64_t)b.nx * b.ny * b.nz; ++i) {
            int32_t x, y, z;
            if (ca_tri_voxel(b, g->radius, i, &x, &y, &z)) g->bits[ca_word_at(g->D, g->W, x >> 6, y, z)] |= 1ull << (x & 63);
        }
    }
    return 0;
}

int hc_cage_fill(const d3ga_voxel_grid *g, int32_t stage, uint64_t *outside, uint64_t *filled, int32_t *changed) {
    const int st = ca_check_fill(g, stage, outside, filled, changed);
    if (st != 0) return st;
    const int32_t D = g->D, W = g->W;
    if (stage == D3GA_CAGE_FILL_BEGIN) {
        for (int32_t z = 0; z < D; ++z)
            for (int32_t y = 0; y < D; ++y)
                for (int32_t w = 0; w < W; ++w) outside[ca_word_at(D, W, w, y, z)] = ca_border_word(g->bits, D, W, w, y, z);
    } else if (stage == D3GA_CAGE_FILL_ROUND) {
        bool any = false;
        for (int32_t z = 0; z < D; ++z)
            for (int32_t y = 0; y < D; ++y) any |= ca_sweep_x(g->bits, outside, D, W, y, z);
        for (int32_t z = 0; z < D; ++z)
            for (int32_t w = 0; w < W; ++w) any |= ca_sweep_line(g->bits, outside, ca_word_at(D, W, w, 0, z), W, D, ca_row_mask(D, w));
        for (int32_t y = 0; y < D; ++y)
            for (int32_t w = 0; w < W; ++w) any |= ca_sweep_line(g->bits, outside, ca_word_at(D, W, w, y, 0), (int64_t)D * W, D, ca_row_mask(D, w));
        if (any) *changed |= 1;
    } else {
        for (int64_t i = 0; i < (int64_t)D * D * W; ++i) filled[i] = ~outside[i] & ca_row_mask(D, (int32_t)(i % W));
    }
    return 0;
}

int64_t hc_cage_iso_scratch_bytes(int32_t radius) { return radius < 1 || radius > kCaMaxRadius ? (int64_t)D3GA_E_SIZE : ca_iso_scratch_bytes(radius); }

int hc_cage_iso_count(const d3ga_voxel_grid *grid, void *scratch, int64_t scratch_bytes, int64_t *counts) {
    const int st = ca_check_iso_count(grid, scratch, scratch_bytes, counts);
    if (st != 0) return st;
    const CaLattice g = {grid->D, grid->W, grid->D + 1, grid->bits};
    const CaIsoScratch sc = ca_iso_carve(scratch, grid->radius);
    int64_t nv = 0, nf = 0, i = 0;
    for (int32_t pz = 0; pz < g.P; ++pz)
        for (int32_t py = 0; py < g.P; ++py)
            for (int32_t px = 0; px < g.P; ++px, ++i) {
                const int cm = ca_corner_mask(g, px, py, pz);
                sc.vstart[i] = (uint32_t)nv;
                nv += ca_popcount7(ca_cross_mask(cm));
                nf += ca_cell_faces(cm);
            }
    counts[0] = nv;
    counts[1] = nf;
    return 0;
}

int hc_cage_iso_emit(const d3ga_voxel_grid *grid, const d3ga_cage_iso_desc *out, void *scratch, int64_t scratch_bytes) {
    const int st = ca_check_iso_emit(grid, out, scratch, scratch_bytes);
    if (st != 0) return st;
    const CaLattice g = {grid->D, grid->W, grid->D + 1, grid->bits};
    const CaIsoScratch sc = ca_iso_carve(scratch, grid->radius);
    const CaIsoMap map = {grid->radius, 0, {out->centre[0], out->centre[1], out->centre[2]}, {out->scale[0], out->scale[1], out->scale[2]}};
    int64_t at = 0, i = 0;
    for (int32_t pz = 0; pz < g.P; ++pz)
        for (int32_t py = 0; py < g.P; ++py)
            for (int32_t px = 0; px < g.P; ++px, ++i) {
                const int32_t p[3] = {px, py, pz};
                const int cm = ca_corner_mask(g, px, py, pz), cross = ca_cross_mask(cm);
                for (int t = 0; t < 7; ++t)
                    if ((cross >> t) & 1) {
                        for (int c = 0; c < 3; ++c) out->vertices[3 * (size_t)sc.vstart[i] + 3 * (size_t)ca_popcount7(cross & ((1 << t) - 1)) + c] = ca_iso_coordinate(map, p[c], t, c);
                    }
                int32_t rows[36];
                const int n = ca_cell_emit(g, sc.vstart, px, py, pz, cm, rows);
                for (int j = 0; j < 3 * n; ++j) out->faces[3 * at + j] = rows[j];
                at += n;
            }
    return 0;
}

int hc_cage_smooth(const d3ga_loop_plan *plan, const d3ga_cage_smooth_desc *smooth) {
    const int st = ca_check_smooth(plan, smooth);
    if (st != 0) return st;
    const d3ga_cage_smooth_desc d = *smooth;
    double *cur = d.x, *next = d.work;
    for (int32_t it = 0; it < d.iterations; ++it) {
        if (d.mode == D3GA_CAGE_SMOOTH_IMPROVED) {
            const GiMesh m = {plan->V, plan->F, cur, d.faces, nullptr};
            for (int32_t v = 0; v < plan->V; ++v) ca_normal(m, d.csr_offsets, d.csr_faces, v, d.normals + 3 * (size_t)v, d.status);
            for (int32_t v = 0; v < plan->V; ++v) ca_improved_step(*plan, cur, d.normals, v, d.lam, next + 3 * (size_t)v, d.status);
            double *t = cur; cur = next; next = t;
        } else {
            for (int32_t v = 0; v < plan->V; ++v) ca_uniform_step(*plan, cur, v, d.lam, next + 3 * (size_t)v, d.status);
            for (int32_t v = 0; v < plan->V; ++v) ca_uniform_step(*plan, next, v, d.mu, cur + 3 * (size_t)v, d.status);
        }
    }
    for (int64_t i = 0; i < 3 * (int64_t)plan->V; ++i) d.out[i] = (float)cur[i];
    return 0;
}

int hc_cage_components(const d3ga_loop_plan *plan, int32_t stage, int32_t *label, int32_t *changed) {
    const int st = ca_check_components(plan, stage, label, changed);
    if (st != 0) return st;
    if (stage == D3GA_CAGE_PARTS_BEGIN) {
        for (int32_t f = 0; f < plan->F; ++f) label[f] = f;
        return 0;
    }
    for (int32_t e = plan->E - 1; e >= 0; --e) {               // any order of arrival: here the last edge first
        int32_t larger, smaller;
        if (!ca_edge_roots(*plan, label, e, &larger, &smaller)) continue;
        if (smaller < label[larger]) label[larger] = smaller;
        *changed |= 1;
    }
    for (int32_t f = 0; f < plan->F; ++f) label[f] = ca_root(label, f);
    return 0;
}
}
