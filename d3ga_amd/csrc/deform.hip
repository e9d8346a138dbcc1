// deform.hip -- cage-side kernels for gfx950: LBS of cage vertices (D0), fused tetrahedral-cage deformation of
// Gaussians forward/backward (D1-D5, A1) and the FEM regulariser (D6).   SURVEY.md sec. 8a.
//
// All three are HBM-streaming, one thread per element, no LDS, no MFMA (no dense contraction on this path).
// Cage vertices (V*12 B, a few hundred KB) and tets (T*16 B) are gathered through L2; the per-Gaussian streams
// (tet id, barycentrics, canonical gradient, scale, rotation -> mean, covariance) are read/written once with
// lane-contiguous addresses.  Gaussians are expected sorted by tet id (static during training), so the four
// corner gathers of neighbouring lanes hit the same cache lines.
#include "d3ga_internal.h"
#include "deform_tail.h"

namespace d3ga {

static_assert(kMergeBlock == kBlock, "the block merge is laid out for the workgroup size");

// 64-lane sum through DPP (see raster_composite.hip); result broadcast from lane 63
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_add_(float v) {
    const int t = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, true);
    return v + __int_as_float(t);
}
__device__ __forceinline__ float wave_sum_(float v) {
    v = dpp_add_<0xB1, 0xf>(v); v = dpp_add_<0x4E, 0xf>(v); v = dpp_add_<0x141, 0xf>(v); v = dpp_add_<0x140, 0xf>(v);
    v = dpp_add_<0x142, 0xa>(v); v = dpp_add_<0x143, 0xc>(v);
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// The same over one 16-lane DPP row: every lane of the row ends with the row's total
__device__ __forceinline__ float row_sum_(float v) {
    v = dpp_add_<0xB1, 0xf>(v); v = dpp_add_<0x4E, 0xf>(v); v = dpp_add_<0x141, 0xf>(v); v = dpp_add_<0x140, 0xf>(v);
    return v;
}

// ---------------------------------------------------------------------------------------------------------
// D0: v' = Rh (sum_k w_k A[idx_k]) [v + delta; 1] + Th
// ---------------------------------------------------------------------------------------------------------
// T = sum_k w_k A[idx_k] (rows 0..2 of the 4x4), k ascending
__device__ __forceinline__ void skin_blend(int v, int K, const float *__restrict__ A, const int32_t *__restrict__ idx,
                                           const float *__restrict__ w, float (&T)[12]) {
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = 0.f;
    for (int k = 0; k < K; ++k) {
        const float wk = w[(size_t)v * K + k];
        const float *a = A + 16 * (size_t)idx[(size_t)v * K + k];
#pragma unroll
        for (int i = 0; i < 12; ++i) T[i] += wk * a[i];
    }
}
__device__ __forceinline__ V3 skin_apply(const float (&T)[12], V3 p) {
    return v3(T[0] * p.x + T[1] * p.y + T[2] * p.z + T[3], T[4] * p.x + T[5] * p.y + T[6] * p.z + T[7],
              T[8] * p.x + T[9] * p.y + T[10] * p.z + T[11]);
}
// Rh^T g (g itself without a global rotation)
__device__ __forceinline__ V3 rot_transposed(const float *__restrict__ Rh, V3 g) {
    if (!Rh) return g;
    return v3(Rh[0] * g.x + Rh[3] * g.y + Rh[6] * g.z, Rh[1] * g.x + Rh[4] * g.y + Rh[7] * g.z,
              Rh[2] * g.x + Rh[5] * g.y + Rh[8] * g.z);
}

__global__ __launch_bounds__(kBlock) void lbs_fwd_kernel(int V, int K, const float *__restrict__ tmpl,
                                                         const float *__restrict__ delta,
                                                         const float *__restrict__ A,
                                                         const int32_t *__restrict__ idx, const float *__restrict__ w,
                                                         const float *__restrict__ Rh, const float *__restrict__ Th,
                                                         float *__restrict__ out) {
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= V) return;
    V3 p = load3(tmpl, v);
    if (delta) p = p + load3(delta, v);
    float T[12];
    skin_blend(v, K, A, idx, w, T);
    V3 o = skin_apply(T, p);
    if (Rh) o = v3(Rh[0] * o.x + Rh[1] * o.y + Rh[2] * o.z, Rh[3] * o.x + Rh[4] * o.y + Rh[5] * o.z,
                   Rh[6] * o.x + Rh[7] * o.y + Rh[8] * o.z);
    if (Th) o = o + v3(Th[0], Th[1], Th[2]);
    out[3 * v] = o.x; out[3 * v + 1] = o.y; out[3 * v + 2] = o.z;
}

__global__ __launch_bounds__(kBlock) void lbs_bwd_kernel(int V, int K, const float *__restrict__ A,
                                                         const int32_t *__restrict__ idx, const float *__restrict__ w,
                                                         const float *__restrict__ Rh, const float *__restrict__ g,
                                                         float *__restrict__ gdelta) {
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= V) return;
    const V3 go = rot_transposed(Rh, load3(g, v));
    float T[12];
    skin_blend(v, K, A, idx, w, T);
    gdelta[3 * v] = T[0] * go.x + T[4] * go.y + T[8] * go.z;
    gdelta[3 * v + 1] = T[1] * go.x + T[5] * go.y + T[9] * go.z;
    gdelta[3 * v + 2] = T[2] * go.x + T[6] * go.y + T[10] * go.z;
}

// Pose gradients of D0 (dL/dA, dL/dRh, dL/dTh; the `pose` argument of d3ga_lbs_cage_bwd and d3ga_cage_deform_bwd).  With
// p~ = [tmpl + delta; 1], T = sum_k w_k A[idx_k], o = T p~ (before Rh), g = dL/dout and g' = Rh^T g:
//   dA_j[0:3,0:4] = sum over the (v,k) with idx = j of w_vk g'_v p~_v^T   (row 3 is never read: exact zeros)
//   dRh = sum_v g_v o_v^T,  dTh = sum_v g_v.
// One launch after the unchanged per-vertex launch of the backward, which leaves g in memory (the upstream gradient itself, or
// the gathered vertex gradient of the fused operator).  By-joint plan (cage_deform.py: lbs_pose_plan, built once per binding):
// entries (V*K) = the flat indices v*K + k of skin_idx sorted by joint (stable), cut into chunks of at most kBlock entries that
// never straddle a joint; chunk_rng (n_chunks) = [begin, end) of each chunk, chunk_ptr (J+1) = the first chunk of each joint.
// Workgroup b < n_chunks sums its chunk (one entry per lane), the next ceil(V / kBlock) workgroups sum (g o^T, g) over kBlock
// vertices each (o recomputed); every workgroup writes 12 partials, and the last one to arrive adds them per joint in chunk
// order (row 3 of dA written 0) and the vertex partials in order for dRh / dTh, then re-arms the plan's counter.  Fixed-order
// sums, no float atomics: bit-reproducible.
__device__ __forceinline__ float block_sum12_(const float (&v)[12], float (*red)[12]) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        const float t = wave_sum_(v[i]);
        if (lane == 0) red[wv][i] = t;
    }
    __syncthreads();
    float s = 0.f;
    if (threadIdx.x < 12)
        for (int k = 0; k < kBlock / 64; ++k) s += red[k][threadIdx.x];
    return s;
}

__global__ __launch_bounds__(kBlock) void lbs_pose_reduce_kernel(
    int V, int K, int J, int n_chunks, const int2 *__restrict__ chunk_rng, const int32_t *__restrict__ chunk_ptr,
    const int32_t *__restrict__ entries, const float *__restrict__ A, const int32_t *__restrict__ idx,
    const float *__restrict__ w, const float *__restrict__ tmpl, const float *__restrict__ delta, const float *__restrict__ Rh,
    const float *__restrict__ g, float *part, unsigned *counter, float *__restrict__ gA, float *__restrict__ gRh,
    float *__restrict__ gTh) {
    __shared__ float red[kBlock / 64][12];
    __shared__ int last;
    const int b = blockIdx.x;
    float ps[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) ps[i] = 0.f;
    if (b < n_chunks) {
        const int2 r = chunk_rng[b];
        const int e = r.x + (int)threadIdx.x;
        if (e < r.y) {
            const int q = entries[e], v = q / K;
            const float wk = w[q];
            V3 p = load3(tmpl, v);
            if (delta) p = p + load3(delta, v);
            const V3 go = rot_transposed(Rh, load3(g, v));
            const V3 wg = v3(wk * go.x, wk * go.y, wk * go.z);
            ps[0] = wg.x * p.x; ps[1] = wg.x * p.y; ps[2] = wg.x * p.z; ps[3] = wg.x;
            ps[4] = wg.y * p.x; ps[5] = wg.y * p.y; ps[6] = wg.y * p.z; ps[7] = wg.y;
            ps[8] = wg.z * p.x; ps[9] = wg.z * p.y; ps[10] = wg.z * p.z; ps[11] = wg.z;
        }
    } else {
        const int v = (b - n_chunks) * kBlock + (int)threadIdx.x;
        if (v < V) {
            V3 p = load3(tmpl, v);
            if (delta) p = p + load3(delta, v);
            float T[12];
            skin_blend(v, K, A, idx, w, T);
            const V3 o = skin_apply(T, p);
            const V3 gv = load3(g, v);
            ps[0] = gv.x * o.x; ps[1] = gv.x * o.y; ps[2] = gv.x * o.z;
            ps[3] = gv.y * o.x; ps[4] = gv.y * o.y; ps[5] = gv.y * o.z;
            ps[6] = gv.z * o.x; ps[7] = gv.z * o.y; ps[8] = gv.z * o.z;
            ps[9] = gv.x; ps[10] = gv.y; ps[11] = gv.z;
        }
    }
    const float s = block_sum12_(ps, red);
    if (threadIdx.x < 64) {                                 // wavefront 0 wrote the partials: it releases them, then counts
        if (threadIdx.x < 12) part[12 * (size_t)b + threadIdx.x] = s;
        __threadfence();
        if (threadIdx.x == 0) last = atomicAdd(counter, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    if (threadIdx.x == 0) *counter = 0u;                    // every other workgroup has counted: re-armed for the next call
    for (int i = threadIdx.x; i < 12 * J; i += kBlock) {    // dA: one element per lane, its chunks in order
        const int j = i / 12, e = i - 12 * j;
        float t = 0.f;
#pragma unroll 8
        for (int c = chunk_ptr[j], ce = chunk_ptr[j + 1]; c < ce; ++c) t += part[12 * (size_t)c + e];
        gA[16 * j + e] = t;
    }
    for (int i = threadIdx.x; i < 4 * J; i += kBlock) gA[16 * (i >> 2) + 12 + (i & 3)] = 0.f;
    // dRh, dTh: 21 lanes per value, each over every 21st vertex partial, then the 21 sums in order
    constexpr int kLanesPerValue = kBlock / 12;
    float t = 0.f;
    if (threadIdx.x < 12 * kLanesPerValue) {
        const int e = threadIdx.x % 12, q = threadIdx.x / 12;
#pragma unroll 4
        for (int c = n_chunks + q; c < (int)gridDim.x; c += kLanesPerValue) t += part[12 * (size_t)c + e];
    }
    __shared__ float vs[kLanesPerValue * 12];
    if (threadIdx.x < 12 * kLanesPerValue) vs[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x < 12) {
        float u = 0.f;
        for (int q = 0; q < kLanesPerValue; ++q) u += vs[12 * q + threadIdx.x];
        if (threadIdx.x < 9) gRh[threadIdx.x] = u;
        else gTh[threadIdx.x - 9] = u;
    }
}

// ---------------------------------------------------------------------------------------------------------
// D1-D5
// ---------------------------------------------------------------------------------------------------------
// (load_deform_in and DeformMerge: deform_tail.h, which also holds the stores and routes below as functions for raster_pre.hip)
__global__ __launch_bounds__(kBlock) void cage_deform_fwd_kernel(int P, const float *__restrict__ tetpoints,
                                                                 const int32_t *__restrict__ tetras,
                                                                 const int32_t *__restrict__ tetra_id,
                                                                 const float *__restrict__ barys,
                                                                 const float *__restrict__ canon_grad,
                                                                 const float *__restrict__ scales,
                                                                 const float *__restrict__ rots,
                                                                 const float *__restrict__ delta_barys, int flags,
                                                                 float *__restrict__ means, float *__restrict__ cov6) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P) return;
    DeformIn in;
    int4 vid;
    load_deform_in(i, tetpoints, tetras, tetra_id, barys, canon_grad, scales, rots, delta_barys, flags, in, vid);
    float m[3], c[6];
    deform_fwd(in, m, c);
    means[3 * (size_t)i] = m[0]; means[3 * (size_t)i + 1] = m[1]; means[3 * (size_t)i + 2] = m[2];
#pragma unroll
    for (int k = 0; k < 6; ++k) cov6[6 * (size_t)i + k] = c[k];
}

__global__ __launch_bounds__(kBlock) void cage_deform_bwd_kernel(
    int P, const float *__restrict__ tetpoints, const int32_t *__restrict__ tetras, const int32_t *__restrict__ tetra_id,
    const float *__restrict__ barys, const float *__restrict__ canon_grad, const float *__restrict__ scales,
    const float *__restrict__ rots, const float *__restrict__ delta_barys, int flags,
    const float *__restrict__ g_means, const float *__restrict__ g_cov6,
    float *__restrict__ g_barys, float *__restrict__ g_scales, float *__restrict__ g_rots, float *__restrict__ corner_grads,
    DeformMerge mg) {
    __shared__ float s_val[3][4 * kBlock];                 // merged path: the workgroup's corner gradients in vertex order
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P && !mg.item_pos) return;
    DeformGrad o;
    int4 vid = make_int4(0, 0, 0, 0);
    if (i < P) {
        DeformIn in;
        load_deform_in(i, tetpoints, tetras, tetra_id, barys, canon_grad, scales, rots, delta_barys, flags, in, vid);
        float gm[3] = {g_means[3 * (size_t)i], g_means[3 * (size_t)i + 1], g_means[3 * (size_t)i + 2]};
        float gc[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) gc[k] = g_cov6[6 * (size_t)i + k];
        deform_bwd(in, gm, gc, o);
        // (the stores and the two routes written out, not called through deform_tail.h's store_deform_grads / deform_merge_epilogue /
        // store_corner_records as the fused raster kernel does: through the calls this kernel compiled to other instruction text --
        // two registers less, another null test and address form -- and it is to stay the kernel it was)
        if (g_barys) reinterpret_cast<float4 *>(g_barys)[i] = make_float4(o.gbary[0], o.gbary[1], o.gbary[2], o.gbary[3]);
        if (g_scales) {
            if (flags & D3GA_DEFORM_LOG_SCALES) {    // d/d(log s) = s * d/ds
                o.gs[0] *= in.s[0]; o.gs[1] *= in.s[1]; o.gs[2] *= in.s[2];
            }
            g_scales[3 * (size_t)i] = o.gs[0]; g_scales[3 * (size_t)i + 1] = o.gs[1]; g_scales[3 * (size_t)i + 2] = o.gs[2];
        }
        if (g_rots) reinterpret_cast<float4 *>(g_rots)[i] = make_float4(o.gq[0], o.gq[1], o.gq[2], o.gq[3]);
    }
    if (mg.item_pos) {
        if (i < P) {
            const ushort4 ps = reinterpret_cast<const ushort4 *>(mg.item_pos)[i];
            s_val[0][ps.x] = o.gx0.x; s_val[1][ps.x] = o.gx0.y; s_val[2][ps.x] = o.gx0.z;
            s_val[0][ps.y] = o.gx1.x; s_val[1][ps.y] = o.gx1.y; s_val[2][ps.y] = o.gx1.z;
            s_val[0][ps.z] = o.gx2.x; s_val[1][ps.z] = o.gx2.y; s_val[2][ps.z] = o.gx2.z;
            s_val[0][ps.w] = o.gx3.x; s_val[1][ps.w] = o.gx3.y; s_val[2][ps.w] = o.gx3.z;
        }
        __syncthreads();
        const int g0 = mg.seg_ptr[blockIdx.x], g1 = mg.seg_ptr[blockIdx.x + 1];
        const int nitems = 4 * min(kBlock, P - (int)blockIdx.x * kBlock);
        for (int g = g0 + (int)threadIdx.x; g < g1; g += kBlock) {
            const int b = mg.seg_begin[g], e = g + 1 < g1 ? (int)mg.seg_begin[g + 1] : nitems;
            float sx = 0.f, sy = 0.f, sz = 0.f;
            for (int k = b; k < e; ++k) { sx += s_val[0][k]; sy += s_val[1][k]; sz += s_val[2][k]; }
            mg.partials[3 * (size_t)g] = sx; mg.partials[3 * (size_t)g + 1] = sy; mg.partials[3 * (size_t)g + 2] = sz;
        }
    } else if (corner_grads) {            // per-corner gradients, summed per vertex by vertex_gather_kernel
        float4 *c = reinterpret_cast<float4 *>(corner_grads + 12 * (size_t)i);
        c[0] = make_float4(o.gx0.x, o.gx0.y, o.gx0.z, o.gx1.x);
        c[1] = make_float4(o.gx1.y, o.gx1.z, o.gx2.x, o.gx2.y);
        c[2] = make_float4(o.gx2.z, o.gx3.x, o.gx3.y, o.gx3.z);
    }
}

// One wavefront per cage vertex: sums the corner gradients of every (Gaussian, corner) incident to the vertex.
// vert_start (V+1) / vert_items (4P, item = 4*gaussian + corner) is the static CSR adjacency built once per cage.
// No atomics, bit-reproducible.
__global__ __launch_bounds__(kBlock) void vertex_gather_kernel(int V, const int32_t *__restrict__ vert_start,
                                                               const int32_t *__restrict__ vert_items,
                                                               const float *__restrict__ corner_grads,
                                                               float *__restrict__ g_tetpoints) {
    const int v = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (v >= V) return;                                       // wave-uniform
    const int lane = threadIdx.x & 63;
    const int b = vert_start[v], e = vert_start[v + 1];
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int k = b + lane; k < e; k += 64) {
        const float *c = corner_grads + 3 * (size_t)vert_items[k];
        sx += c[0]; sy += c[1]; sz += c[2];
    }
    sx = wave_sum_(sx); sy = wave_sum_(sy); sz = wave_sum_(sz);
    if (lane == 0) { g_tetpoints[3 * (size_t)v] = sx; g_tetpoints[3 * (size_t)v + 1] = sy; g_tetpoints[3 * (size_t)v + 2] = sz; }
}

// The same with ONE DPP ROW (16 lanes) per vertex, four vertices per wavefront: for short item lists -- the partials of the
// block-merged backward, two to four per vertex with coherent numbering -- a whole wavefront per vertex leaves 60 lanes idle
// and the launch is 4x the wavefronts (7.3 -> .. us at C3).
// LBS (round 5): the LBS backward of D0 behind the gather -- the posed cage vertices came from d3ga_lbs_cage_fwd, so
// dL/d(delta) = (sum_k w_k A_k[:3,:3])^T Rh^T dL/d(tetpoint) is formed while the vertex gradient sits in the row's registers: one
// launch instead of two for ~24 k vertices.  Lane k of the row takes joint k of the vertex.  g_extra: a gradient that reaches
// the vertices by another route (the FEM regulariser), added before the skinning; g_tetpoints is then optional.
template <bool LBS>
__global__ __launch_bounds__(kBlock) void vertex_gather_row_kernel(int V, int K, const int32_t *__restrict__ vert_start,
                                                                   const int32_t *__restrict__ vert_items,
                                                                   const float *__restrict__ values,
                                                                   const float *__restrict__ g_extra,
                                                                   const float *__restrict__ A, const int32_t *__restrict__ idx,
                                                                   const float *__restrict__ w, const float *__restrict__ Rh,
                                                                   float *__restrict__ g_tetpoints, float *__restrict__ gdelta) {
    const int v = blockIdx.x * (kBlock / 16) + (threadIdx.x >> 4);
    const int l16 = threadIdx.x & 15;
    const bool live = v < V;
    const int b = live ? vert_start[v] : 0, e = live ? vert_start[v + 1] : 0;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int k = b + l16; k < e; k += 16) {
        const float *c = values + 3 * (size_t)vert_items[k];
        sx += c[0]; sy += c[1]; sz += c[2];
    }
    if (LBS && g_extra && live && l16 == 0) { sx += g_extra[3 * (size_t)v]; sy += g_extra[3 * (size_t)v + 1]; sz += g_extra[3 * (size_t)v + 2]; }
    sx = row_sum_(sx); sy = row_sum_(sy); sz = row_sum_(sz);
    if ((!LBS || g_tetpoints) && live && l16 == 0) { g_tetpoints[3 * (size_t)v] = sx; g_tetpoints[3 * (size_t)v + 1] = sy; g_tetpoints[3 * (size_t)v + 2] = sz; }
    if constexpr (LBS) {
        const V3 go = rot_transposed(Rh, v3(sx, sy, sz));
        float dx = 0.f, dy = 0.f, dz = 0.f;
        if (live) {
            for (int k = l16; k < K; k += 16) {
                const float wk = w[(size_t)v * K + k];
                const float *a = A + 16 * (size_t)idx[(size_t)v * K + k];
                dx += wk * (a[0] * go.x + a[4] * go.y + a[8] * go.z);
                dy += wk * (a[1] * go.x + a[5] * go.y + a[9] * go.z);
                dz += wk * (a[2] * go.x + a[6] * go.y + a[10] * go.z);
            }
        }
        dx = row_sum_(dx); dy = row_sum_(dy); dz = row_sum_(dz);
        if (live && l16 == 0) { gdelta[3 * (size_t)v] = dx; gdelta[3 * (size_t)v + 1] = dy; gdelta[3 * (size_t)v + 2] = dz; }
    }
}

// ---------------------------------------------------------------------------------------------------------
// D6
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void atomic_add3(float *base, int v, V3 g) {
    atomicAdd(base + 3 * (size_t)v, g.x);
    atomicAdd(base + 3 * (size_t)v + 1, g.y);
    atomicAdd(base + 3 * (size_t)v + 2, g.z);
}

__global__ __launch_bounds__(kBlock) void fem_fwd_kernel(int T, const float *__restrict__ tetpoints,
                                                         const int32_t *__restrict__ tetras,
                                                         const float *__restrict__ Dn_inv, float *__restrict__ energy) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= T) return;
    const int4 vid = reinterpret_cast<const int4 *>(tetras)[t];
    M3 D;
#pragma unroll
    for (int k = 0; k < 9; ++k) D.m[k] = Dn_inv[9 * (size_t)t + k];
    energy[t] = fem_energy_fwd(load3(tetpoints, vid.x), load3(tetpoints, vid.y), load3(tetpoints, vid.z),
                               load3(tetpoints, vid.w), D);
}
__global__ __launch_bounds__(kBlock) void fem_bwd_kernel(int T, const float *__restrict__ tetpoints,
                                                         const int32_t *__restrict__ tetras,
                                                         const float *__restrict__ Dn_inv, const float *__restrict__ g,
                                                         float *__restrict__ g_tetpoints) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= T) return;
    const int4 vid = reinterpret_cast<const int4 *>(tetras)[t];
    M3 D;
#pragma unroll
    for (int k = 0; k < 9; ++k) D.m[k] = Dn_inv[9 * (size_t)t + k];
    V3 gx[4];
    fem_energy_bwd(load3(tetpoints, vid.x), load3(tetpoints, vid.y), load3(tetpoints, vid.z), load3(tetpoints, vid.w),
                   D, g[t], gx);
    atomic_add3(g_tetpoints, vid.x, gx[0]); atomic_add3(g_tetpoints, vid.y, gx[1]);
    atomic_add3(g_tetpoints, vid.z, gx[2]); atomic_add3(g_tetpoints, vid.w, gx[3]);
}

}  // namespace d3ga

using namespace d3ga;

static inline int nblocks(int n) { return (n + kBlock - 1) / kBlock; }

extern "C" int d3ga_lbs_cage_fwd(int V, int K, const float *tmpl, const float *delta, const float *joint_mats,
                                 const int32_t *skin_idx, const float *skin_w, const float *Rh, const float *Th,
                                 float *out, d3ga_stream_t stream) {
    if (V < 0 || K <= 0) return D3GA_E_SIZE;
    if (V == 0) return D3GA_OK;
    if (!tmpl || !joint_mats || !skin_idx || !skin_w || !out) return D3GA_E_NULL;
    hipLaunchKernelGGL(lbs_fwd_kernel, dim3(nblocks(V)), dim3(kBlock), 0, (hipStream_t)stream, V, K, tmpl, delta,
                       joint_mats, skin_idx, skin_w, Rh, Th, out);
    return check_launch((hipStream_t)stream, 0);
}

// scratch of the pose backward: partials (12 per workgroup of the reduction) | the fused operator's vertex gradient (3V)
static int64_t pose_groups(int V, int n_chunks) { return (int64_t)n_chunks + (V + kBlock - 1) / kBlock; }

extern "C" int d3ga_lbs_pose_scratch_bytes(int V, int32_t n_chunks, int32_t fused, int64_t *bytes) {
    if (V < 0 || n_chunks < 0) return D3GA_E_SIZE;
    if (!bytes) return D3GA_E_NULL;
    *bytes = 4 * (12 * pose_groups(V, n_chunks) + (fused ? 3 * (int64_t)V : 0));
    return D3GA_OK;
}

static int pose_check(int V, int K, const d3ga_lbs_pose_grad *pg) {
    if (pg->J <= 0 || pg->n_chunks <= 0 || (int64_t)V * K != pg->n_entries) return D3GA_E_SIZE;
    if (!pg->tmpl || !pg->chunk_ptr || !pg->chunk_range || !pg->entries || !pg->counter || !pg->scratch || !pg->g_joint_mats ||
        !pg->g_Rh || !pg->g_Th)
        return D3GA_E_NULL;
    if (((uintptr_t)pg->chunk_range & 7) || ((uintptr_t)pg->scratch & 3)) return D3GA_E_CONFIG;     // int2 / float reads
    return D3GA_OK;
}

static int pose_reduce(int V, int K, const float *joint_mats, const int32_t *skin_idx, const float *skin_w, const float *Rh,
                       const float *g, const d3ga_lbs_pose_grad *pg, hipStream_t s) {
    hipLaunchKernelGGL(lbs_pose_reduce_kernel, dim3((unsigned)pose_groups(V, pg->n_chunks)), dim3(kBlock), 0, s, V, K, pg->J,
                       pg->n_chunks, (const int2 *)pg->chunk_range, pg->chunk_ptr, pg->entries, joint_mats, skin_idx, skin_w,
                       pg->tmpl, pg->delta, Rh, g, (float *)pg->scratch, (unsigned *)pg->counter, pg->g_joint_mats, pg->g_Rh,
                       pg->g_Th);
    return check_launch(s, 0);
}

extern "C" int d3ga_lbs_cage_bwd(int V, int K, const float *joint_mats, const int32_t *skin_idx, const float *skin_w,
                                 const float *Rh, const float *grad_out, float *grad_delta, const d3ga_lbs_pose_grad *pose,
                                 d3ga_stream_t stream) {
    if (V < 0 || K <= 0 || (pose && V == 0)) return D3GA_E_SIZE;
    if (V == 0) return D3GA_OK;
    if (pose) D3GA_TRY(pose_check(V, K, pose));
    if (!joint_mats || !skin_idx || !skin_w || !grad_out || !grad_delta) return D3GA_E_NULL;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(lbs_bwd_kernel, dim3(nblocks(V)), dim3(kBlock), 0, s, V, K, joint_mats, skin_idx, skin_w, Rh, grad_out,
                       grad_delta);
    D3GA_TRY(check_launch(s, 0));
    return pose ? pose_reduce(V, K, joint_mats, skin_idx, skin_w, Rh, grad_out, pose, s) : D3GA_OK;
}

// what the forward and the backward kernel both read
static int deform_in_check(const d3ga_cage_deform_in *in) {
    return (!in->tetpoints || !in->tetras || !in->tetra_id || !in->barys || !in->canon_grad || !in->scales || !in->rots)
               ? D3GA_E_NULL : D3GA_OK;
}

extern "C" int d3ga_cage_deform_fwd(const d3ga_cage_deform_in *in, float *means3D, float *cov6, d3ga_stream_t stream) {
    if (!in) return D3GA_E_NULL;
    if (in->flags & ~(D3GA_DEFORM_LOG_SCALES | D3GA_DEFORM_GRAD_PER_TET)) return D3GA_E_CONFIG;
    if (in->P < 0) return D3GA_E_SIZE;
    if (in->P == 0) return D3GA_OK;
    D3GA_TRY(deform_in_check(in));
    if (!means3D || !cov6) return D3GA_E_NULL;
    hipLaunchKernelGGL(cage_deform_fwd_kernel, dim3(nblocks(in->P)), dim3(kBlock), 0, (hipStream_t)stream, in->P, in->tetpoints,
                       in->tetras, in->tetra_id, in->barys, in->canon_grad, in->scales, in->rots, in->delta_barys, (int)in->flags,
                       means3D, cov6);
    return check_launch((hipStream_t)stream, 0);
}

// One validation, one launch of cage_deform_bwd_kernel, then the vertex gather the route asks for (with the skinning backward in
// it when `skin` is given) and the by-joint reduction of `pose`.  tail_only (d3ga_cage_deform_bwd_tail): the route's records are
// already filled -- by the per-Gaussian raster backward that ran the deform backward as its tail -- and the kernel is not launched.
static int cage_deform_bwd(const d3ga_cage_deform_in *in, const d3ga_cage_deform_grads *gr, const d3ga_cage_deform_route *route,
                           const d3ga_cage_deform_skin *skin, const d3ga_lbs_pose_grad *pose, d3ga_stream_t stream, bool tail_only) {
    if (!in || !gr) return D3GA_E_NULL;
    const int P = in->P, V = in->V;
    const bool merge = route && route->kind == D3GA_DEFORM_ROUTE_MERGE, corners = route && route->kind == D3GA_DEFORM_ROUTE_CORNERS;
    if (P < 0 || V < 0 || (merge && route->n_segments < 0) || (skin && skin->K <= 0) || (pose && V == 0)) return D3GA_E_SIZE;
    if ((in->flags & ~(D3GA_DEFORM_LOG_SCALES | D3GA_DEFORM_GRAD_PER_TET)) || (route && !merge && !corners) || (skin && !merge) ||
        (pose && !skin))
        return D3GA_E_CONFIG;
    if (pose) D3GA_TRY(pose_check(V, skin->K, pose));
    if (skin) {
        if (!skin->g_delta || !skin->joint_mats || !skin->skin_idx || !skin->skin_w) return D3GA_E_NULL;
        if (V == 0) return D3GA_OK;
    } else if (P > 0 && (route != nullptr) != (gr->g_tetpoints != nullptr)) {
        return D3GA_E_NULL;              // a route needs its output, and g_tetpoints has no other way (no float atomics)
    }
    hipStream_t s = (hipStream_t)stream;
    // the vertex gradient: the caller's g_tetpoints, or (pose) the scratch behind the partials of the reduction
    float *gv = (pose && !gr->g_tetpoints) ? (float *)pose->scratch + 12 * pose_groups(V, pose->n_chunks) : gr->g_tetpoints;
    if (P == 0) {
        if (!skin) {
            if (gv && V > 0) D3GA_HIP(zero_async(gv, sizeof(float) * 3 * (size_t)V, s));
            return D3GA_OK;
        }
        // no Gaussian, no segment: the gather reads vert_start (V+1 zeros) alone, vert_items / records may be the NULL of an
        // empty tensor
        if (route->n_segments != 0) return D3GA_E_SIZE;
        if (!route->vert_start) return D3GA_E_NULL;
    } else if (tail_only) {
        if (route && (!route->vert_start || !route->vert_items || !route->records)) return D3GA_E_NULL;
    } else {
        D3GA_TRY(deform_in_check(in));
        if (!gr->g_means || !gr->g_cov6 || (route && (!route->vert_start || !route->vert_items || !route->records)) ||
            (merge && (!route->item_pos || !route->seg_ptr || !route->seg_begin)))
            return D3GA_E_NULL;
        if (merge && ((uintptr_t)route->item_pos & 7)) return D3GA_E_CONFIG;  // read 8 bytes per Gaussian
        hipLaunchKernelGGL(cage_deform_bwd_kernel, dim3(nblocks(P)), dim3(kBlock), 0, s, P, in->tetpoints, in->tetras, in->tetra_id,
                           in->barys, in->canon_grad, in->scales, in->rots, in->delta_barys, (int)in->flags, gr->g_means, gr->g_cov6,
                           gr->g_barys, gr->g_scales, gr->g_rots, corners ? route->records : nullptr,
                           merge ? DeformMerge{route->item_pos, route->seg_ptr, route->seg_begin, route->records}
                                 : DeformMerge{nullptr, nullptr, nullptr, nullptr});
        D3GA_TRY(check_launch(s, 0));
    }
    if (!route || V == 0) return D3GA_OK;
    const dim3 rows((V + kBlock / 16 - 1) / (kBlock / 16));
    if (skin)
        hipLaunchKernelGGL(vertex_gather_row_kernel<true>, rows, dim3(kBlock), 0, s, V, skin->K, route->vert_start, route->vert_items,
                           (const float *)route->records, skin->g_tetpoints_extra, skin->joint_mats, skin->skin_idx, skin->skin_w,
                           skin->Rh, gv, skin->g_delta);
    else if (merge && (int64_t)route->n_segments <= 24 * (int64_t)V)      // short lists (the usual case): a DPP row per vertex
        hipLaunchKernelGGL(vertex_gather_row_kernel<false>, rows, dim3(kBlock), 0, s, V, 0, route->vert_start, route->vert_items,
                           (const float *)route->records, (const float *)nullptr, (const float *)nullptr, (const int32_t *)nullptr,
                           (const float *)nullptr, (const float *)nullptr, gv, (float *)nullptr);
    else
        hipLaunchKernelGGL(vertex_gather_kernel, dim3((V + 3) / 4), dim3(kBlock), 0, s, V, route->vert_start, route->vert_items,
                           (const float *)route->records, gv);
    D3GA_TRY(check_launch(s, 0));
    return pose ? pose_reduce(V, skin->K, skin->joint_mats, skin->skin_idx, skin->skin_w, skin->Rh, gv, pose, s) : D3GA_OK;
}

extern "C" int d3ga_cage_deform_bwd(const d3ga_cage_deform_in *in, const d3ga_cage_deform_grads *gr,
                                    const d3ga_cage_deform_route *route, const d3ga_cage_deform_skin *skin,
                                    const d3ga_lbs_pose_grad *pose, d3ga_stream_t stream) {
    return cage_deform_bwd(in, gr, route, skin, pose, stream, false);
}

extern "C" int d3ga_cage_deform_bwd_tail(const d3ga_cage_deform_in *in, const d3ga_cage_deform_grads *gr,
                                         const d3ga_cage_deform_route *route, const d3ga_cage_deform_skin *skin,
                                         const d3ga_lbs_pose_grad *pose, d3ga_stream_t stream) {
    return cage_deform_bwd(in, gr, route, skin, pose, stream, true);
}

// What the fused raster backward checks of its deform arguments before it launches (d3ga_raster_preprocess_bwd_deform): the
// rules of d3ga_cage_deform_bwd for the kernel's own inputs, outputs and route.
int d3ga::deform_tail_check(const d3ga_cage_deform_in *in, const d3ga_cage_deform_grads *gr, const d3ga_cage_deform_route *route) {
    if (!in || !gr) return D3GA_E_NULL;
    const bool merge = route && route->kind == D3GA_DEFORM_ROUTE_MERGE, corners = route && route->kind == D3GA_DEFORM_ROUTE_CORNERS;
    if (in->P < 0 || in->V < 0 || (merge && route->n_segments < 0)) return D3GA_E_SIZE;
    if ((in->flags & ~(D3GA_DEFORM_LOG_SCALES | D3GA_DEFORM_GRAD_PER_TET)) || (route && !merge && !corners)) return D3GA_E_CONFIG;
    if (in->P == 0) return D3GA_OK;
    D3GA_TRY(deform_in_check(in));
    if ((route && !route->records) || (merge && (!route->item_pos || !route->seg_ptr || !route->seg_begin))) return D3GA_E_NULL;
    if (merge && ((uintptr_t)route->item_pos & 7)) return D3GA_E_CONFIG;  // read 8 bytes per Gaussian
    return D3GA_OK;
}

extern "C" int d3ga_fem_energy_fwd(int T, const float *tetpoints, const int32_t *tetras, const float *Dn_inv,
                                   float *energy, d3ga_stream_t stream) {
    if (T < 0) return D3GA_E_SIZE;
    if (T == 0) return D3GA_OK;
    if (!tetpoints || !tetras || !Dn_inv || !energy) return D3GA_E_NULL;
    hipLaunchKernelGGL(fem_fwd_kernel, dim3(nblocks(T)), dim3(kBlock), 0, (hipStream_t)stream, T, tetpoints, tetras,
                       Dn_inv, energy);
    return check_launch((hipStream_t)stream, 0);
}

extern "C" int d3ga_fem_energy_bwd(int T, int V, const float *tetpoints, const int32_t *tetras, const float *Dn_inv,
                                   const float *g_energy, float *g_tetpoints, d3ga_stream_t stream) {
    if (T < 0 || V < 0) return D3GA_E_SIZE;
    if (!g_tetpoints) return D3GA_E_NULL;
    if (V > 0) D3GA_HIP(zero_async(g_tetpoints, sizeof(float) * 3 * (size_t)V, (hipStream_t)stream));
    if (T == 0) return D3GA_OK;
    if (!tetpoints || !tetras || !Dn_inv || !g_energy) return D3GA_E_NULL;
    hipLaunchKernelGGL(fem_bwd_kernel, dim3(nblocks(T)), dim3(kBlock), 0, (hipStream_t)stream, T, tetpoints, tetras,
                       Dn_inv, g_energy, g_tetpoints);
    return check_launch((hipStream_t)stream, 0);
}
