// bary_interp.hip -- barycentric interpolation of per-row attributes over a static binding, for gfx950 (include/d3ga.h, D2b).
//
// A binding is one table rows (P,K) int32: corner k of Gaussian i reads row rows[i,k] of attr (V,C).  K = 4 is the cage binding
// (tetras[tetra_id], optionally seen through a vertex map), K = 3 the mesh binding (the face's three vertex ids per Gaussian).
//
// THE SUMMATION ORDERS (the specification of record; DESIGN.md sec. 4.4k derives the error bounds from them):
//   forward     w_k = barys[i,k] + delta_barys[i,k]  (one rounding; w_k = barys[i,k] as it is without delta_barys)
//               out[i,c] = fma(w_{K-1}, a_{K-1}, ... fma(w_1, a_1, w_0 * a_0)),  a_k = attr[rows[i,k], c]: k ascending.
//   g_barys     g_barys[i,k] = fma(a_{C-1}, g_{C-1}, ... fma(a_1, g_1, a_0 * g_0)),  a_c = attr[rows[i,k], c], g_c = g_out[i,c]:
//               c ascending, per Gaussian.
//   g_attr      a GATHER over the CSR lists vert_start (V+1) / vert_items (K P; item q = K i + k), 16 lanes (one DPP row's worth)
//               per row v of attr, four rows per wavefront.  With b = vert_start[v], lane l (0..15) sums the items at list
//               positions b + l, b + l + 16, b + l + 32, ... in that order:  s = 0;  s = fma(w_q, g_out[i,c], s)  with w_q rounded
//               as in the forward.  The sixteen lane sums are then added by a butterfly over lane distance 1, 2, 4, 8 (s += the
//               partner's s), so the total is ((l0+l1)+(l2+l3)) + ... pairwise.  An empty list gives +0.  The order depends on
//               the lists alone: no float atomics, two calls on the same inputs are bit-identical, and every row of g_attr is
//               written by the call.
//
// All three kernels are gather-bound with short dependent chains: one thread per Gaussian (or 16 lanes per row), every
// independent load (ids, weights, the K C gathered values) issued before the first use, registers only, no LDS.  The weights of
// a missing delta_barys are read a second time from barys (the same cache line) so that the loads stay unconditional.
#include "d3ga_internal.h"

namespace d3ga {

template <int K>
__device__ __forceinline__ void bary_load_rows(int64_t i, const int32_t *__restrict__ rows, int (&r)[K]) {
    if constexpr (K == 4) {
        const int4 v = reinterpret_cast<const int4 *>(rows)[i];
        r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) r[k] = rows[K * i + k];
    }
}

// w_k = barys + delta_barys (one rounding), or barys as it is
template <int K>
__device__ __forceinline__ void bary_load_weights(int64_t i, const float *__restrict__ barys, const float *__restrict__ delta,
                                                  float (&w)[K]) {
    const float *second = delta ? delta : barys;
    float b[K], d[K];
    if constexpr (K == 4) {
        const float4 vb = reinterpret_cast<const float4 *>(barys)[i], vd = reinterpret_cast<const float4 *>(second)[i];
        b[0] = vb.x; b[1] = vb.y; b[2] = vb.z; b[3] = vb.w;
        d[0] = vd.x; d[1] = vd.y; d[2] = vd.z; d[3] = vd.w;
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) { b[k] = barys[K * i + k]; d[k] = second[K * i + k]; }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) w[k] = delta ? b[k] + d[k] : b[k];
}

template <int K, int C>
__device__ __forceinline__ void bary_gather(const float *__restrict__ attr, const int (&r)[K], float (&a)[K][C]) {
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int c = 0; c < C; ++c) a[k][c] = attr[(size_t)r[k] * C + c];
}

template <int K, int C>
__global__ __launch_bounds__(kBlock) void bary_interp_fwd_kernel(int P, const float *__restrict__ attr,
                                                                 const int32_t *__restrict__ rows,
                                                                 const float *__restrict__ barys,
                                                                 const float *__restrict__ delta, float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= P) return;
    int r[K];
    float w[K], a[K][C];
    bary_load_rows<K>(i, rows, r);
    bary_load_weights<K>(i, barys, delta, w);
    bary_gather<K, C>(attr, r, a);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float s = w[0] * a[0][c];
#pragma unroll
        for (int k = 1; k < K; ++k) s = fmaf(w[k], a[k][c], s);
        out[(size_t)i * C + c] = s;
    }
}

template <int K, int C>
__global__ __launch_bounds__(kBlock) void bary_interp_gbarys_kernel(int P, const float *__restrict__ attr,
                                                                    const int32_t *__restrict__ rows,
                                                                    const float *__restrict__ g_out,
                                                                    float *__restrict__ g_barys) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= P) return;
    int r[K];
    float g[C], a[K][C], s[K];
    bary_load_rows<K>(i, rows, r);
#pragma unroll
    for (int c = 0; c < C; ++c) g[c] = g_out[(size_t)i * C + c];
    bary_gather<K, C>(attr, r, a);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        s[k] = a[k][0] * g[0];
#pragma unroll
        for (int c = 1; c < C; ++c) s[k] = fmaf(a[k][c], g[c], s[k]);
    }
    if constexpr (K == 4) {
        reinterpret_cast<float4 *>(g_barys)[i] = make_float4(s[0], s[1], s[2], s[3]);
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) g_barys[K * i + k] = s[k];
    }
}

constexpr int kBaryLanes = 16;      // lanes per row of attr in the gather
constexpr int kBaryAhead = 4;       // list items a lane has in flight

template <int K, int C>
__global__ __launch_bounds__(kBlock) void bary_interp_gattr_kernel(int V, const int32_t *__restrict__ vert_start,
                                                                   const int32_t *__restrict__ vert_items,
                                                                   const float *__restrict__ barys,
                                                                   const float *__restrict__ delta,
                                                                   const float *__restrict__ g_out, float *__restrict__ g_attr) {
    const int64_t v = (int64_t)blockIdx.x * (kBlock / kBaryLanes) + (threadIdx.x / kBaryLanes);
    const int l = threadIdx.x % kBaryLanes;
    const bool live = v < V;
    const int b = live ? vert_start[v] : 0, e = live ? vert_start[v + 1] : 0;
    const float *second = delta ? delta : barys;
    float s[C];
#pragma unroll
    for (int c = 0; c < C; ++c) s[c] = 0.f;
    for (int p0 = b + l; p0 < e; p0 += kBaryLanes * kBaryAhead) {
        int q[kBaryAhead];
        float wb[kBaryAhead], wd[kBaryAhead], g[kBaryAhead][C];
#pragma unroll
        for (int u = 0; u < kBaryAhead; ++u) {              // a position beyond the list reads the lane's first item again
            const int p = p0 + kBaryLanes * u;
            q[u] = vert_items[p < e ? p : p0];
        }
#pragma unroll
        for (int u = 0; u < kBaryAhead; ++u) {
            const size_t i = (size_t)(q[u] / K);
            wb[u] = barys[q[u]];
            wd[u] = second[q[u]];
#pragma unroll
            for (int c = 0; c < C; ++c) g[u][c] = g_out[i * C + c];
        }
#pragma unroll
        for (int u = 0; u < kBaryAhead; ++u) {
            if (p0 + kBaryLanes * u < e) {
                const float w = delta ? wb[u] + wd[u] : wb[u];
#pragma unroll
                for (int c = 0; c < C; ++c) s[c] = fmaf(w, g[u][c], s[c]);
            }
        }
    }
    // every lane of the wavefront is here again: the sixteen lane sums, by a butterfly inside the group of 16
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int off = 1; off < kBaryLanes; off <<= 1) s[c] += __shfl_xor(s[c], off, kBaryLanes);
    if (live && l == 0) {
#pragma unroll
        for (int c = 0; c < C; ++c) g_attr[(size_t)v * C + c] = s[c];
    }
}

template <int K, int C>
static void bary_launch_fwd(hipStream_t s, int P, const float *attr, const int32_t *rows, const float *barys, const float *delta,
                            float *out) {
    hipLaunchKernelGGL((bary_interp_fwd_kernel<K, C>), dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0, s, P, attr, rows, barys,
                       delta, out);
}
template <int K, int C>
static void bary_launch_gbarys(hipStream_t s, int P, const float *attr, const int32_t *rows, const float *g_out, float *g_barys) {
    hipLaunchKernelGGL((bary_interp_gbarys_kernel<K, C>), dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0, s, P, attr, rows, g_out,
                       g_barys);
}
template <int K, int C>
static void bary_launch_gattr(hipStream_t s, int V, const int32_t *vert_start, const int32_t *vert_items, const float *barys,
                              const float *delta, const float *g_out, float *g_attr) {
    constexpr int per = kBlock / kBaryLanes;
    hipLaunchKernelGGL((bary_interp_gattr_kernel<K, C>), dim3((V + per - 1) / per), dim3(kBlock), 0, s, V, vert_start, vert_items,
                       barys, delta, g_out, g_attr);
}

}  // namespace d3ga

using namespace d3ga;

// FN<K, C>(...) for the runtime (K, C) of the domain K in {3, 4}, 1 <= C <= 8
#define D3GA_BARY_FOR_C(FN, K, C, ...)                                                                                   \
    switch (C) {                                                                                                          \
        case 1: FN<K, 1>(__VA_ARGS__); break;                                                                             \
        case 2: FN<K, 2>(__VA_ARGS__); break;                                                                             \
        case 3: FN<K, 3>(__VA_ARGS__); break;                                                                             \
        case 4: FN<K, 4>(__VA_ARGS__); break;                                                                             \
        case 5: FN<K, 5>(__VA_ARGS__); break;                                                                             \
        case 6: FN<K, 6>(__VA_ARGS__); break;                                                                             \
        case 7: FN<K, 7>(__VA_ARGS__); break;                                                                             \
        default: FN<K, 8>(__VA_ARGS__); break;                                                                            \
    }
#define D3GA_BARY_DISPATCH(FN, K, C, ...)                                                                                \
    do {                                                                                                                  \
        if ((K) == 3) { D3GA_BARY_FOR_C(FN, 3, C, __VA_ARGS__) } else { D3GA_BARY_FOR_C(FN, 4, C, __VA_ARGS__) }          \
    } while (0)

static int bary_domain(int64_t P, int64_t V, int K, int C) {
    return (P < 0 || V < 0 || (K != 3 && K != 4) || C < 1 || C > 8 || P * K > INT32_MAX) ? D3GA_E_SIZE : D3GA_OK;
}
// K == 4 reads and writes 16 bytes per Gaussian
static bool bary_misaligned(int K, const void *a, const void *b, const void *c, const void *d) {
    return K == 4 && ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) != 0);
}

extern "C" int d3ga_bary_interp_fwd(int32_t P, int32_t K, int32_t C, const float *attr, const int32_t *rows, const float *barys,
                                    const float *delta_barys, float *out, d3ga_stream_t stream) {
    D3GA_TRY(bary_domain(P, 0, K, C));
    if (P == 0) return D3GA_OK;
    if (!attr || !rows || !barys || !out) return D3GA_E_NULL;
    if (bary_misaligned(K, rows, barys, delta_barys, nullptr)) return D3GA_E_CONFIG;
    hipStream_t s = (hipStream_t)stream;
    D3GA_BARY_DISPATCH(bary_launch_fwd, K, C, s, P, attr, rows, barys, delta_barys, out);
    return check_launch(s, 0);
}

extern "C" int d3ga_bary_interp_bwd(int32_t P, int32_t V, int32_t K, int32_t C, const float *attr, const int32_t *rows,
                                    const float *barys, const float *delta_barys, const float *g_out, const int32_t *vert_start,
                                    const int32_t *vert_items, float *g_attr, float *g_barys, d3ga_stream_t stream) {
    D3GA_TRY(bary_domain(P, V, K, C));
    hipStream_t s = (hipStream_t)stream;
    if (P == 0) {                                       // no item: every list is empty
        if (g_attr && V > 0) D3GA_HIP(zero_async(g_attr, sizeof(float) * (size_t)V * C, s));
        return D3GA_OK;
    }
    if (!attr || !rows || !barys || !g_out || (g_attr && (!vert_start || !vert_items))) return D3GA_E_NULL;
    if (bary_misaligned(K, rows, barys, delta_barys, g_barys)) return D3GA_E_CONFIG;
    if (g_barys) {
        D3GA_BARY_DISPATCH(bary_launch_gbarys, K, C, s, P, attr, rows, g_out, g_barys);
        D3GA_TRY(check_launch(s, 0));
    }
    if (g_attr && V > 0) {
        D3GA_BARY_DISPATCH(bary_launch_gattr, K, C, s, V, vert_start, vert_items, barys, delta_barys, g_out, g_attr);
        D3GA_TRY(check_launch(s, 0));
    }
    return D3GA_OK;
}
