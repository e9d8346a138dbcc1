// knn.hip -- K nearest neighbours with distances and indices: pytorch3d's knn_points as the reference calls it
// (models/cage_net.py:21,66: knn_points(points[None], points[None], K = 4)), forward only.  Semantics: DESIGN.md 4.4j; the
// arithmetic is csrc/knn_math.h, which the tests also build with g++ (this file is compiled with -ffp-contract=off).
//
// One query per lane; the K (distance, index) slots live in registers (knn_insert indexes them statically).  K is a template
// parameter in {1, 2, 4, 8, 16}; a requested K is rounded up and the first K slots are stored.
//   exhaustive: every workgroup streams p2 through LDS in blocks of 256 points, as knn3_mean_dist2_kernel (bary.hip) does;
//   grid:       p2 bucketed into a uniform grid by the caller; a query walks the Chebyshev rings around its (clamped) cell, as
//               knn3_grid_kernel does, and stops once its K-th pair lies strictly inside the query's true distance to the
//               planes that bound the visited block of cells (knn_axis_reach) -- a query need not be a member of p2 nor lie
//               inside its box.  Both kernels insert the same (distance, index) pairs into an order-independent structure, so
//               they return the same bits.
#include "d3ga_internal.h"
#include "knn_math.h"

namespace d3ga {

template <int K>
__global__ __launch_bounds__(kBlock) void knn_points_kernel(int P1, int P2, int k_out, const float *__restrict__ p1,
                                                            const float *__restrict__ p2, float *__restrict__ dists,
                                                            int64_t *__restrict__ idx) {
    __shared__ float s_p[kBlock * 3];
    const int tid = threadIdx.x;
    const int i = blockIdx.x * kBlock + tid;
    const size_t n = blockIdx.y;                              // batch element
    const bool live = i < P1;
    const float *q = p1 + (n * (size_t)P1 + (size_t)(live ? i : 0)) * 3;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (live) { px = q[0]; py = q[1]; pz = q[2]; }
    const float *cloud = p2 + n * (size_t)P2 * 3;
    float d[K];
    int32_t id[K];
    knn_clear<K>(d, id);
    for (int base = 0; base < P2; base += kBlock) {
        const int cnt = min(kBlock, P2 - base);
        __syncthreads();
        for (int k = tid; k < cnt * 3; k += kBlock) s_p[k] = cloud[(size_t)base * 3 + k];
        __syncthreads();
        if (!live) continue;
        for (int j = 0; j < cnt; ++j) knn_consider<K>(d, id, s_p + 3 * j, px, py, pz, base + j);
    }
    if (live) {
        const size_t row = (n * (size_t)P1 + (size_t)i) * (size_t)k_out;
        knn_store<K>(d, id, k_out, dists + row, idx + row);
    }
}

template <int K>
__global__ __launch_bounds__(kBlock) void knn_points_grid_kernel(int P1, int P2, int k_out, const float *__restrict__ p1,
                                                                 const float *__restrict__ p2,
                                                                 const int32_t *__restrict__ cell_start,
                                                                 const int32_t *__restrict__ cell_points, float ox, float oy,
                                                                 float oz, float h, int nx, int ny, int nz,
                                                                 float *__restrict__ dists, int64_t *__restrict__ idx) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P1) return;
    const float px = p1[3 * (size_t)i], py = p1[3 * (size_t)i + 1], pz = p1[3 * (size_t)i + 2];
    float d[K];
    int32_t id[K];
    knn_clear<K>(d, id);
    knn_grid_search<K>(px, py, pz, P2, p2, cell_start, cell_points, ox, oy, oz, h, nx, ny, nz, d, id);
    const size_t row = (size_t)i * (size_t)k_out;
    knn_store<K>(d, id, k_out, dists + row, idx + row);
}

static inline int knn_sizes(int N, int P1, int P2, int K) {
    if (N < 0 || P1 < 0 || P2 < 0 || P2 == 0x7fffffff || N > 65535) return D3GA_E_SIZE;
    if (K < 1 || K > kKnnMaxK) return D3GA_E_SIZE;
    return D3GA_OK;
}

}  // namespace d3ga

using namespace d3ga;

#define D3GA_KNN_DISPATCH(K, LAUNCH)      \
    do {                                  \
        if ((K) <= 1) { LAUNCH(1); }      \
        else if ((K) <= 2) { LAUNCH(2); } \
        else if ((K) <= 4) { LAUNCH(4); } \
        else if ((K) <= 8) { LAUNCH(8); } \
        else { LAUNCH(16); }              \
    } while (0)

extern "C" int d3ga_knn_points(int N, int P1, int P2, int K, const float *p1, const float *p2, float *dists, int64_t *idx,
                               d3ga_stream_t stream) {
    D3GA_TRY(knn_sizes(N, P1, P2, K));
    if (N == 0 || P1 == 0) return D3GA_OK;
    if (!p1 || !dists || !idx || (P2 > 0 && !p2)) return D3GA_E_NULL;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((P1 + kBlock - 1) / kBlock), (unsigned)N);
#define D3GA_KNN_LAUNCH(KT) hipLaunchKernelGGL(knn_points_kernel<KT>, grid, dim3(kBlock), 0, s, P1, P2, K, p1, p2, dists, idx)
    D3GA_KNN_DISPATCH(K, D3GA_KNN_LAUNCH);
#undef D3GA_KNN_LAUNCH
    return check_launch(s, 0);
}

extern "C" int d3ga_knn_points_grid(int P1, int P2, int K, const float *p1, const float *p2, const int32_t *cell_start,
                                    const int32_t *cell_points, const float *origin_h, const int32_t *dims, float *dists,
                                    int64_t *idx, d3ga_stream_t stream) {
    D3GA_TRY(knn_sizes(1, P1, P2, K));
    if (P1 == 0) return D3GA_OK;
    if (!p1 || !dists || !idx || !cell_start || !origin_h || !dims || (P2 > 0 && (!p2 || !cell_points))) return D3GA_E_NULL;
    if (dims[0] <= 0 || dims[1] <= 0 || dims[2] <= 0 || !(origin_h[3] > 0.f) || !(origin_h[3] <= 3.0e38f)) return D3GA_E_SIZE;
    if ((int64_t)dims[0] * dims[1] * dims[2] >= ((int64_t)1 << 31) - 1) return D3GA_E_SIZE;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((P1 + kBlock - 1) / kBlock));
#define D3GA_KNN_LAUNCH(KT)                                                                                                  \
    hipLaunchKernelGGL(knn_points_grid_kernel<KT>, grid, dim3(kBlock), 0, s, P1, P2, K, p1, p2, cell_start, cell_points, origin_h[0], \
                       origin_h[1], origin_h[2], origin_h[3], dims[0], dims[1], dims[2], dists, idx)
    D3GA_KNN_DISPATCH(K, D3GA_KNN_LAUNCH);
#undef D3GA_KNN_LAUNCH
    return check_launch(s, 0);
}
