// deform_tail.h -- the cage deformation's backward for the per-Gaussian raster backward that runs it as its tail (raster_pre.hip:
// preprocess_bwd_kernel<., true>): the loads of one Gaussian's deform inputs (load_deform_in and DeformMerge also serve deform.hip),
// the stores of its per-Gaussian gradients and the two routes of its corner gradients.  cage_deform_bwd_kernel (deform.hip) has the
// stores and the routes written out in its own body -- the same statements: called from here it compiled to other instruction text.
//
// The index arithmetic of the block merge (D3GA_HD) also compiles with a host compiler: tests/hostcheck/deform_tail_host.cpp walks it
// against a scalar reference under the sanitizers.
#pragma once
#include "d3ga_math.h"

namespace d3ga {

constexpr int kMergeBlock = 256;       // Gaussians per workgroup of the block merge (= kBlock; cage_deform.py: _MERGE_BLOCK)
constexpr int kMergeItems = 4 * kMergeBlock;

// Block-level merge of the corner gradients (round 4; D3GA_DEFORM_ROUTE_MERGE).  The binding is static, so for every
// workgroup of 256 consecutive Gaussians the positions of its 1024 (Gaussian, corner) items in vertex-sorted order
// (item_pos), the segments of equal vertex (seg_ptr / seg_begin) and where each segment's sum goes (partial g = global
// segment index) are built ONCE (cage_deform.py: merge_plan).  The kernel drops its corner gradients into LDS at those
// positions, sums every segment in a fixed order (no atomics: bit-reproducible) and writes one partial per (workgroup,
// vertex) -- with spatially coherent numbering a few hundred per workgroup instead of 1024 corner records; the vertex
// gather then runs over the partials.
struct DeformMerge {
    const uint16_t *item_pos;      // (P,4)  position of item 4 i + c among its workgroup's items sorted by vertex
    const int32_t *seg_ptr;        // (workgroups + 1)  first global segment of each workgroup
    const uint16_t *seg_begin;     // (segments)  first position of the segment inside its workgroup
    float *partials;               // (segments,3)
};

// one Gaussian's four corner gradients into the workgroup's planes, at its items' positions p0..p3
D3GA_HD void deform_merge_put(float (&s_val)[3][kMergeItems], unsigned p0, unsigned p1, unsigned p2, unsigned p3,
                              const DeformGrad &o) {
    s_val[0][p0] = o.gx0.x; s_val[1][p0] = o.gx0.y; s_val[2][p0] = o.gx0.z;
    s_val[0][p1] = o.gx1.x; s_val[1][p1] = o.gx1.y; s_val[2][p1] = o.gx1.z;
    s_val[0][p2] = o.gx2.x; s_val[1][p2] = o.gx2.y; s_val[2][p2] = o.gx2.z;
    s_val[0][p3] = o.gx3.x; s_val[1][p3] = o.gx3.y; s_val[2][p3] = o.gx3.z;
}
// items of workgroup `block` (the last one may be partial)
D3GA_HD int deform_merge_items(int P, int block) {
    const int left = P - block * kMergeBlock;
    return 4 * (kMergeBlock < left ? kMergeBlock : left);
}
// thread `tid` of workgroup `block`: the sums of its segments (tid, tid + 256, ..), each in position order, into the partials
D3GA_HD void deform_merge_sums(const float (&s_val)[3][kMergeItems], const DeformMerge &mg, int P, int block, int tid) {
    const int g0 = mg.seg_ptr[block], g1 = mg.seg_ptr[block + 1];
    const int nitems = deform_merge_items(P, block);
    for (int g = g0 + tid; g < g1; g += kMergeBlock) {
        const int b = mg.seg_begin[g], e = g + 1 < g1 ? (int)mg.seg_begin[g + 1] : nitems;
        float sx = 0.f, sy = 0.f, sz = 0.f;
        for (int k = b; k < e; ++k) { sx += s_val[0][k]; sy += s_val[1][k]; sz += s_val[2][k]; }
        mg.partials[3 * (size_t)g] = sx; mg.partials[3 * (size_t)g + 1] = sy; mg.partials[3 * (size_t)g + 2] = sz;
    }
}

#ifdef __HIPCC__
__device__ __forceinline__ V3 load3(const float *p, int i) { return v3(p[3 * i], p[3 * i + 1], p[3 * i + 2]); }

// The inputs of Gaussian i in two parts: the dependent chain tetra_id -> tetras -> tetpoints (three round trips deep, through L2;
// -> the tetrahedron), and the per-Gaussian streams -- for a caller that puts other work between them.  load_deform_in below is
// the two in one.
__device__ __forceinline__ int load_deform_corners(int i, const float *tetpoints, const int32_t *tetras,
                                                   const int32_t *tetra_id, DeformIn &in, int4 &vid) {
    const int t = tetra_id[i];
    vid = reinterpret_cast<const int4 *>(tetras)[t];
    in.x0 = load3(tetpoints, vid.x); in.x1 = load3(tetpoints, vid.y);
    in.x2 = load3(tetpoints, vid.z); in.x3 = load3(tetpoints, vid.w);
    return t;
}
__device__ __forceinline__ void load_deform_streams(int i, int t, const float *barys, const float *canon_grad,
                                                    const float *scales, const float *rots,
                                                    const float *delta_barys, int flags, DeformIn &in) {
    const float4 b = reinterpret_cast<const float4 *>(barys)[i];
    in.bary[0] = b.x; in.bary[1] = b.y; in.bary[2] = b.z; in.bary[3] = b.w;
    if (delta_barys) {                       // canon_barys = barys + delta_bary (models/cage_net.py:213), fused
        const float4 d = reinterpret_cast<const float4 *>(delta_barys)[i];
        in.bary[0] += d.x; in.bary[1] += d.y; in.bary[2] += d.z; in.bary[3] += d.w;
    }
    // the canonical gradient is a property of the TETRAHEDRON: per Gaussian as the reference stores it (lib/cage.py:329,
    // 36 B x P streamed per pass), or -- D3GA_DEFORM_GRAD_PER_TET -- one (T,3,3) table read through tetra_id (L2-resident)
    const size_t gi = (flags & D3GA_DEFORM_GRAD_PER_TET) ? (size_t)t : (size_t)i;
#pragma unroll
    for (int k = 0; k < 9; ++k) in.G.m[k] = canon_grad[9 * gi + k];
    in.s[0] = scales[3 * (size_t)i]; in.s[1] = scales[3 * (size_t)i + 1]; in.s[2] = scales[3 * (size_t)i + 2];
    if (flags & D3GA_DEFORM_LOG_SCALES) {    // scales = exp(scaling) (models/cage_net.py:214), fused
        in.s[0] = expf(in.s[0]); in.s[1] = expf(in.s[1]); in.s[2] = expf(in.s[2]);
    }
    const float4 q = reinterpret_cast<const float4 *>(rots)[i];
    in.q[0] = q.x; in.q[1] = q.y; in.q[2] = q.z; in.q[3] = q.w;
}
__device__ __forceinline__ void load_deform_in(int i, const float *__restrict__ tetpoints,
                                               const int32_t *__restrict__ tetras, const int32_t *__restrict__ tetra_id,
                                               const float *__restrict__ barys, const float *__restrict__ canon_grad,
                                               const float *__restrict__ scales, const float *__restrict__ rots,
                                               const float *__restrict__ delta_barys, int flags, DeformIn &in,
                                               int4 &vid) {
    // (the two parts written out, not called: through the calls cage_deform_fwd_kernel's exp() chain was scheduled differently)
    const int t = tetra_id[i];
    vid = reinterpret_cast<const int4 *>(tetras)[t];
    in.x0 = load3(tetpoints, vid.x); in.x1 = load3(tetpoints, vid.y);
    in.x2 = load3(tetpoints, vid.z); in.x3 = load3(tetpoints, vid.w);
    const float4 b = reinterpret_cast<const float4 *>(barys)[i];
    in.bary[0] = b.x; in.bary[1] = b.y; in.bary[2] = b.z; in.bary[3] = b.w;
    if (delta_barys) {
        const float4 d = reinterpret_cast<const float4 *>(delta_barys)[i];
        in.bary[0] += d.x; in.bary[1] += d.y; in.bary[2] += d.z; in.bary[3] += d.w;
    }
    const size_t gi = (flags & D3GA_DEFORM_GRAD_PER_TET) ? (size_t)t : (size_t)i;
#pragma unroll
    for (int k = 0; k < 9; ++k) in.G.m[k] = canon_grad[9 * gi + k];
    in.s[0] = scales[3 * (size_t)i]; in.s[1] = scales[3 * (size_t)i + 1]; in.s[2] = scales[3 * (size_t)i + 2];
    if (flags & D3GA_DEFORM_LOG_SCALES) {
        in.s[0] = expf(in.s[0]); in.s[1] = expf(in.s[1]); in.s[2] = expf(in.s[2]);
    }
    const float4 q = reinterpret_cast<const float4 *>(rots)[i];
    in.q[0] = q.x; in.q[1] = q.y; in.q[2] = q.z; in.q[3] = q.w;
}

// the per-Gaussian gradients of Gaussian i, each where wanted (o.gs is left with the log-scale chain applied)
__device__ __forceinline__ void store_deform_grads(int i, int flags, const DeformIn &in, DeformGrad &o, float *__restrict__ g_barys,
                                                   float *__restrict__ g_scales, float *__restrict__ g_rots) {
    if (g_barys) reinterpret_cast<float4 *>(g_barys)[i] = make_float4(o.gbary[0], o.gbary[1], o.gbary[2], o.gbary[3]);
    if (g_scales) {
        if (flags & D3GA_DEFORM_LOG_SCALES) {    // d/d(log s) = s * d/ds
            o.gs[0] *= in.s[0]; o.gs[1] *= in.s[1]; o.gs[2] *= in.s[2];
        }
        g_scales[3 * (size_t)i] = o.gs[0]; g_scales[3 * (size_t)i + 1] = o.gs[1]; g_scales[3 * (size_t)i + 2] = o.gs[2];
    }
    if (g_rots) reinterpret_cast<float4 *>(g_rots)[i] = make_float4(o.gq[0], o.gq[1], o.gq[2], o.gq[3]);
}

// The merge epilogue.  EVERY thread of the workgroup must call it (live: this thread has a Gaussian, i < P): the LDS scatter by
// item_pos, the barrier, the fixed-order segment sums.
__device__ __forceinline__ void deform_merge_epilogue(float (&s_val)[3][kMergeItems], const DeformMerge &mg, int P, int i, bool live,
                                                      const DeformGrad &o) {
    if (live) {
        const ushort4 ps = reinterpret_cast<const ushort4 *>(mg.item_pos)[i];
        deform_merge_put(s_val, ps.x, ps.y, ps.z, ps.w, o);
    }
    __syncthreads();
    deform_merge_sums(s_val, mg, P, (int)blockIdx.x, (int)threadIdx.x);
}

// per-corner gradients of Gaussian i (D3GA_DEFORM_ROUTE_CORNERS), summed per vertex by vertex_gather_kernel
__device__ __forceinline__ void store_corner_records(float *__restrict__ corner_grads, int i, const DeformGrad &o) {
    float4 *c = reinterpret_cast<float4 *>(corner_grads + 12 * (size_t)i);
    c[0] = make_float4(o.gx0.x, o.gx0.y, o.gx0.z, o.gx1.x);
    c[1] = make_float4(o.gx1.y, o.gx1.z, o.gx2.x, o.gx2.y);
    c[2] = make_float4(o.gx2.z, o.gx3.x, o.gx3.y, o.gx3.z);
}
#endif  // __HIPCC__

}  // namespace d3ga
