// CPU build of d3ga_amd/csrc/template_bind_math.h: the argument rules and the per-element text of template_bind.hip, walked in
// the kernels' order of stages (keys; heads, their exclusive prefix, the edge rows and the counts; the offsets; the neighbour lists
// filled and sorted; the stencils; the faces; unpose).  Built by tests/template_bind_ref.py with -ffp-contract=off.
#include "../../d3ga_amd/csrc/template_bind_math.h"

using namespace d3ga;

extern "C" {

int64_t hc_loop_plan_scratch_bytes(int32_t V, int32_t F) { return tb_check_sizes(V, F) != 0 ? (int64_t)D3GA_E_SIZE : tb_scratch_bytes(V, F); }

// same arguments as d3ga_loop_edge_keys (include/d3ga.h), host memory
int hc_loop_edge_keys(int32_t V, int32_t F, const int32_t *faces, int64_t *keys, uint32_t *status) {
    const int st = tb_check_keys(V, F, faces, keys, status);
    if (st != 0) return st;
    for (int64_t h = 0; h < 3 * (int64_t)F; ++h) keys[h] = tb_edge_key(V, faces, h, status);
    return 0;
}

static void scan(int64_t n, const int32_t *vals, int32_t *excl) {
    int32_t run = 0;
    for (int64_t i = 0; i < n; ++i) { excl[i] = run; run += vals[i]; }
    excl[n] = run;
}

// same arguments as d3ga_loop_plan_build
int hc_loop_plan_build(const d3ga_loop_plan *plan, const int32_t *faces, const int64_t *keys, const int64_t *perm, int32_t *info, void *scratch,
                       int64_t scratch_bytes) {
    const int st = tb_check_build(plan, faces, keys, perm, info, scratch, scratch_bytes);
    if (st != 0) return st;
    const int32_t V = plan->V;
    const int64_t n = 3 * (int64_t)plan->F;
    const TbScratch sc = tb_carve(scratch, V, plan->F);
    uint32_t *status = reinterpret_cast<uint32_t *>(info + 2);
    for (int32_t v = 0; v < V; ++v) { sc.valence[v] = 0; sc.cursor[v] = 0; plan->vert_boundary[v] = 0; }
    info[0] = info[1] = 0;
    for (int64_t p = 0; p < n; ++p) sc.head[p] = tb_is_head(keys, p);
    scan(n, sc.head, sc.excl);
    info[0] = sc.excl[n];
    for (int64_t p = 0; p < n; ++p) {
        const int64_t h = perm[p];
        if ((uint64_t)h >= (uint64_t)n) { *status |= D3GA_BIND_STATUS_RANGE; continue; }
        if (keys[p] == kTbBadKey) { plan->face_edge[h] = -1; continue; }
        const int32_t e = sc.head[p] ? sc.excl[p] : sc.excl[p] - 1;
        if (e < 0 || (int64_t)e >= n) continue;
        plan->face_edge[h] = e;
        if (!sc.head[p]) continue;
        const TbEdge ed = tb_edge_at(V, n, keys, perm, faces, p, status);
        plan->edge_verts[2 * (size_t)e] = ed.lo;  plan->edge_verts[2 * (size_t)e + 1] = ed.hi;
        plan->edge_opp[2 * (size_t)e] = ed.o0;    plan->edge_opp[2 * (size_t)e + 1] = ed.o1;
        plan->edge_faces[2 * (size_t)e] = ed.f0;  plan->edge_faces[2 * (size_t)e + 1] = ed.f1;
        plan->edge_boundary[e] = ed.boundary ? 1 : 0;
        if (ed.lo < 0) continue;
        ++sc.valence[ed.lo];
        ++sc.valence[ed.hi];
        if (ed.boundary) { plan->vert_boundary[ed.lo] = 1; plan->vert_boundary[ed.hi] = 1; }
    }
    scan(V, sc.valence, plan->vert_offsets);
    for (int32_t e = info[0] - 1; e >= 0; --e) {              // any order of arrival: here the last edge first
        const int32_t lo = plan->edge_verts[2 * (size_t)e], hi = plan->edge_verts[2 * (size_t)e + 1];
        if ((uint32_t)lo >= (uint32_t)V || (uint32_t)hi >= (uint32_t)V) continue;
        const int32_t a = plan->vert_offsets[lo] + sc.cursor[lo]++, b = plan->vert_offsets[hi] + sc.cursor[hi]++;
        if (a < plan->vert_offsets[lo + 1]) plan->vert_nbr[a] = hi;
        if (b < plan->vert_offsets[hi + 1]) plan->vert_nbr[b] = lo;
    }
    for (int32_t v = 0; v < V; ++v) {
        tb_sort_segment(plan->vert_nbr, plan->vert_offsets[v], plan->vert_offsets[v + 1]);
        const int32_t k = plan->vert_offsets[v + 1] - plan->vert_offsets[v];
        if (k > info[1]) info[1] = k;
    }
    return 0;
}

int hc_loop_subdivide(const d3ga_loop_plan *plan, int32_t D, const double *x, const double *beta, int32_t n_beta, float *out, uint32_t *status) {
    const int st = tb_check_subdivide(plan, D, x, beta, n_beta, out, status);
    if (st != 0) return st;
    const int64_t total = ((int64_t)plan->V + plan->E) * D;
    for (int64_t i = 0; i < total; ++i) out[i] = tb_stencil(*plan, x, D, i, beta, n_beta, status);
    return 0;
}

int hc_loop_faces(const d3ga_loop_plan *plan, const int32_t *faces, int32_t *out) {
    const int st = tb_check_faces(plan, faces, out);
    if (st != 0) return st;
    for (int32_t f = 0; f < plan->F; ++f) tb_face_rows(*plan, faces, f, out + 12 * (size_t)f);
    return 0;
}

int hc_unpose(int32_t n, int32_t J, int32_t R, int32_t K, const double *vertices, const double *joint_mats, const void *skin_w, int32_t w_f64,
              const int32_t *skin_idx, const int64_t *rows, const double *offsets, int32_t n_offsets, float *out, uint32_t *status) {
    const int st = tb_check_unpose(n, J, R, K, vertices, joint_mats, skin_w, w_f64, skin_idx, rows, offsets, n_offsets, out, status);
    if (st != 0) return st;
    const TbUnpose u = {n, J, R, K, n_offsets, vertices, joint_mats, offsets, skin_idx, rows};
    for (int32_t i = 0; i < n; ++i) {
        if (w_f64) tb_unpose_one<double>(u, static_cast<const double *>(skin_w), i, out + 3 * (size_t)i, status);
        else tb_unpose_one<float>(u, static_cast<const float *>(skin_w), i, out + 3 * (size_t)i, status);
    }
    return 0;
}
}
