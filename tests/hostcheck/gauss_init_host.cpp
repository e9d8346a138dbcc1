// CPU build of d3ga_amd/csrc/gauss_init_math.h: the argument rules and the per-face / per-sample / per-vertex text of
// gauss_init.hip, walked in the kernels' layout (blocks of kGiBlock faces, an inclusive scan inside each, the exclusive prefix of
// the block totals).  Built by tests/gauss_init_ref.py with -ffp-contract=off.
#include "../../d3ga_amd/csrc/gauss_init_math.h"

using namespace d3ga;

extern "C" {

int64_t hc_surface_sample_scratch_bytes(int32_t F) { return gi_scratch_bytes(F); }

// same arguments as d3ga_surface_sample (include/d3ga.h), host memory
int hc_surface_sample(int32_t V, int32_t F, int32_t n, const double *verts, const int32_t *faces, const uint8_t *face_mask,
                      const double *uniforms, float *points, float *rotations, int32_t *out_faces, int32_t *face_id, float *barys, void *scratch,
                      int64_t scratch_bytes, uint32_t *status, int32_t block) {
    const int st = gi_check_sample(V, F, n, verts, faces, face_mask, uniforms, points, rotations, out_faces, face_id, barys, scratch,
                                   scratch_bytes, status, block);
    if (st != 0) return st;
    const GiMesh m = {V, F, verts, faces, face_mask};
    const GiScratch sc = gi_carve(scratch, F);
    const int64_t nblk = gi_blocks(F);
    uint64_t max_bits = 0;
    for (int f = 0; f < F; ++f) {
        bool bad = false;
        const uint64_t b = gi_bits(gi_area(m, f, &bad));
        if (bad) *status |= D3GA_SAMPLE_STATUS_RANGE;
        if (b > max_bits) max_bits = b;
    }
    *sc.max_bits = max_bits;
    const int k = gi_shift(max_bits, F);
    for (int64_t b = 0; b < nblk; ++b) {
        uint64_t run = 0;
        for (int f = (int)(b * kGiBlock); f < F && f < (b + 1) * kGiBlock; ++f) {
            bool bad = false;
            run += gi_quantize(gi_area(m, f, &bad), k);
            sc.cum_local[f] = run;
        }
        sc.block_total[b] = run;
    }
    uint64_t carry = 0;
    for (int64_t b = 0; b < nblk; ++b) {
        sc.block_start[b] = carry;
        carry += sc.block_total[b];
    }
    sc.block_start[nblk] = carry;
    if (carry == 0) *status |= D3GA_SAMPLE_STATUS_EMPTY;
    for (int i = 0; i < n; ++i) {
        GiSample s = GiSample{};
        s.face_id = -1;
        if (carry != 0) s = gi_sample(m, sc.cum_local, sc.block_start, carry, uniforms + 3 * (size_t)i);
        for (int c = 0; c < 3; ++c) {
            points[3 * (size_t)i + c] = s.point[c];
            out_faces[3 * (size_t)i + c] = s.face[c];
            barys[3 * (size_t)i + c] = s.bary[c];
        }
        for (int c = 0; c < 4; ++c) rotations[4 * (size_t)i + c] = s.quat[c];
        face_id[i] = s.face_id;
    }
    return 0;
}

// the integer weights of a call: cum (F) uint64 inclusive, *shift = k
int hc_surface_weights(int32_t F, const void *scratch, uint64_t *cum, uint64_t *max_bits) {
    const GiScratch sc = gi_carve(const_cast<void *>(scratch), F);
    for (int f = 0; f < F; ++f) cum[f] = gi_cum(sc.cum_local, sc.block_start, f);
    *max_bits = *sc.max_bits;
    return gi_shift(*sc.max_bits, F);
}

int hc_vertex_normals_angle(int32_t V, int32_t F, const double *verts, const int32_t *faces, const int32_t *csr_offsets,
                            const int32_t *csr_faces, double amount, double *normals, double *inflated, uint32_t *status) {
    const int st = gi_check_normals(V, F, verts, faces, csr_offsets, csr_faces, amount, normals, inflated, status);
    if (st != 0) return st;
    const GiMesh m = {V, F, verts, faces, nullptr};
    for (int v = 0; v < V; ++v) {
        bool bad = false;
        const GiVec nv = gi_vertex_normal(m, csr_offsets, csr_faces, v, &bad);
        if (bad) *status |= D3GA_SAMPLE_STATUS_RANGE;
        const double c[3] = {nv.x, nv.y, nv.z};
        for (int a = 0; a < 3; ++a) {
            if (normals) normals[3 * (size_t)v + a] = c[a];
            if (inflated) inflated[3 * (size_t)v + a] = verts[3 * (size_t)v + a] + amount * c[a];
        }
    }
    return 0;
}
}
