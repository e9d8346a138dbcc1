// pose_prior.hip -- the pose prior: the PCA of the refined poses and the clamp that every driven frame goes
// through before it conditions the field networks.
//   pose_fit_*   test.py:264-274 + utils/pca_utils.py:14-24 (sklearn PCA.fit): the float64 column mean and covariance of the
//                (N,D) table of refined poses, which already lives on the device (FramePoses.optimizable_poses.table).  The
//                eigen-solve of the (D,D) matrix, D <= 256, once per run, is the host's (LAPACK in float64 is the yardstick).
//   pose_clamp   test.py:49-56, 88-92 (transform_pca): project on the k components, clip every coefficient to sigma standard
//                deviations, project back -- a device-to-host copy, scikit-learn on the CPU and a host-to-device copy per frame
//                there; ONE launch here, a workgroup per pose, the row read through a device index when asked.
//
// The arithmetic and its summation orders are pose_prior_math.h's (this file is built with -ffp-contract=off, so the g++
// build of that header is a bit-level yardstick).  Nothing here uses an atomic.
//
// Fit: a chunk is kPoseFitChunk rows WHATEVER the launch looks like, so the partial sums -- and the result -- do not depend on
// the geometry.  Mean: thread = column, a workgroup per chunk.  Covariance: a workgroup is a 16 x 16 tile of C for one chunk;
// the two 16-column strips of the centred rows go through LDS 32 rows at a time, every thread adds its product row by row.
// Only tiles on or above the diagonal are computed (x_i x_j = x_j x_i bit for bit); the finish kernel mirrors them.
//
// Clamp: D, k <= 256 = one workgroup.  The centred pose is staged in LDS; projection lanes run over j and read the (D,k) copy
// of the basis, reconstruction lanes run over d and read the (k,D) copy: consecutive lanes read consecutive doubles both
// times, and the LDS operand is a broadcast.  Each lane's sum is serial in the pinned order: a chain of D (then k) float64
// multiply-adds whose loads do not depend on it.  The call is bound by its launch, not by this chain.
#include "d3ga_internal.h"
#include "pose_prior_math.h"

namespace d3ga {

static_assert(kPoseMaxD <= kBlock, "one thread per column / component");
constexpr int kCovTile = 16;                     // a workgroup's tile of C: 16 x 16 = kBlock threads
constexpr int kCovRows = 32;                     // rows staged in LDS per round
static_assert(kCovTile * kCovTile == kBlock, "a thread per element of the tile");

__global__ __launch_bounds__(kBlock) void pose_mean_partial_kernel(const float *__restrict__ table, int N, int D,
                                                                    double *__restrict__ pmean) {
    const int col = threadIdx.x;
    if (col >= D) return;
    const int r0 = blockIdx.x * kPoseFitChunk, r1 = min(r0 + kPoseFitChunk, N);
    pmean[(size_t)blockIdx.x * D + col] = pp_chunk_sum(table, D, r0, r1, col);
}

__global__ __launch_bounds__(kBlock) void pose_mean_finish_kernel(const double *__restrict__ pmean, int N, int D, int chunks,
                                                                   double *__restrict__ out) {
    const int col = threadIdx.x;
    if (col >= D) return;
    out[col] = pp_chunks_total(pmean + col, (size_t)D, chunks, (double)N);
}

__global__ __launch_bounds__(kBlock) void pose_cov_partial_kernel(const float *__restrict__ table, const double *__restrict__ mean,
                                                                   int N, int D, int tiles, double *__restrict__ pcov) {
    __shared__ double s_i[kCovRows][kCovTile];
    __shared__ double s_j[kCovRows][kCovTile];
    const int bi = blockIdx.y / tiles, bj = blockIdx.y - bi * tiles;
    if (bj < bi) return;                                     // (uniform) below the diagonal: mirrored by the finish kernel
    const int tid = threadIdx.x, tx = tid & (kCovTile - 1), ty = tid / kCovTile;
    const int r0 = blockIdx.x * kPoseFitChunk, r1 = min(r0 + kPoseFitChunk, N);
    double acc = 0.0;
    for (int rb = r0; rb < r1; rb += kCovRows) {
        const int nr = min(kCovRows, r1 - rb);
        __syncthreads();                                     // the previous round's reads are done
        for (int e = tid; e < nr * kCovTile; e += kBlock) {
            const int rr = e / kCovTile, cc = e & (kCovTile - 1);
            const int ci = bi * kCovTile + cc, cj = bj * kCovTile + cc;
            const size_t row = (size_t)(rb + rr) * D;
            s_i[rr][cc] = ci < D ? pp_centre(table[row + ci], mean[ci]) : 0.0;
            s_j[rr][cc] = cj < D ? pp_centre(table[row + cj], mean[cj]) : 0.0;
        }
        __syncthreads();
        for (int rr = 0; rr < nr; ++rr) acc = pp_cov_step(acc, s_i[rr][ty], s_j[rr][tx]);
    }
    const int i = bi * kCovTile + ty, j = bj * kCovTile + tx;
    if (i < D && j < D) pcov[(size_t)blockIdx.x * D * D + (size_t)i * D + j] = acc;
}

__global__ __launch_bounds__(kBlock) void pose_cov_finish_kernel(const double *__restrict__ pcov, int N, int D, int chunks,
                                                                  double *__restrict__ cov) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= D * D) return;
    const int i = e / D, j = e - i * D;
    const int src = i / kCovTile <= j / kCovTile ? e : j * D + i;     // the tile that was computed
    cov[e] = pp_chunks_total(pcov + src, (size_t)D * D, chunks, (double)(N - 1));
}

// One workgroup per pose.  ROWS: the pose is row rows[b] of the table `in`.
template <bool ROWS>
__global__ __launch_bounds__(kBlock) void pose_clamp_kernel(const float *__restrict__ in, const int32_t *__restrict__ rows, int n_rows,
                                                             int D, int k, const double *__restrict__ mean,
                                                             const double *__restrict__ comp, const double *__restrict__ comp_t,
                                                             const double *__restrict__ std, double sigma, int stages,
                                                             float *__restrict__ out, int32_t *__restrict__ flag) {
    __shared__ double s_x[kPoseMaxD];
    __shared__ double s_z[kPoseMaxD];
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    int64_t src = b;
    if constexpr (ROWS) {
        const int r = rows[b];
        if (r < 0 || r >= n_rows) {                          // (uniform) nothing of output row b is written
            if (tid == 0) flag[0] = 1;
            return;
        }
        src = r;
    }
    const bool project = stages & D3GA_POSE_STAGE_PROJECT, reconstruct = stages & D3GA_POSE_STAGE_RECONSTRUCT;
    if (project) {
        if (tid < D) s_x[tid] = pp_centre(in[src * D + tid], mean[tid]);
        __syncthreads();
        if (tid < k) {
            double z = pp_project(s_x, comp_t, D, k, tid);
            if (stages & D3GA_POSE_STAGE_CLIP) z = pp_clip(z, sigma, std[tid]);
            if (reconstruct) s_z[tid] = z;
            else out[(int64_t)b * k + tid] = (float)z;
        }
    } else if (tid < k) s_z[tid] = (double)in[src * k + tid];
    if (!reconstruct) return;
    __syncthreads();
    if (tid < D) out[(int64_t)b * D + tid] = pp_reconstruct(s_z, comp, mean, D, k, tid);
}

}  // namespace d3ga

using namespace d3ga;

static inline int pose_fit_shape(int32_t N, int32_t D) {
    if (N < 2 || D < 1 || D > D3GA_POSE_MAX_D || (int64_t)N * D > INT32_MAX) return D3GA_E_SIZE;
    return 0;
}

extern "C" int d3ga_pose_fit_scratch_bytes(int32_t N, int32_t D, int64_t *bytes) {
    if (!bytes) return D3GA_E_NULL;
    D3GA_TRY(pose_fit_shape(N, D));
    *bytes = (int64_t)pp_chunks(N) * ((int64_t)D + (int64_t)D * D) * (int64_t)sizeof(double);
    return D3GA_OK;
}

extern "C" int d3ga_pose_fit(const float *table, int32_t N, int32_t D, double *out, void *scratch, d3ga_stream_t stream) {
    D3GA_TRY(pose_fit_shape(N, D));
    if (!table || !out || !scratch) return D3GA_E_NULL;
    if (((uintptr_t)scratch | (uintptr_t)out) & 7) return D3GA_E_CONFIG;
    const int chunks = pp_chunks(N);
    const int tiles = (D + kCovTile - 1) / kCovTile;
    double *pmean = (double *)scratch, *pcov = pmean + (size_t)chunks * D;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(pose_mean_partial_kernel, dim3(chunks), dim3(kBlock), 0, s, table, N, D, pmean);
    hipLaunchKernelGGL(pose_mean_finish_kernel, dim3(1), dim3(kBlock), 0, s, (const double *)pmean, N, D, chunks, out);
    hipLaunchKernelGGL(pose_cov_partial_kernel, dim3(chunks, tiles * tiles), dim3(kBlock), 0, s, table, (const double *)out, N, D,
                       tiles, pcov);
    hipLaunchKernelGGL(pose_cov_finish_kernel, dim3((D * D + kBlock - 1) / kBlock), dim3(kBlock), 0, s, (const double *)pcov, N, D,
                       chunks, out + D);
    return check_launch(s, 0);
}

extern "C" int d3ga_pose_clamp(const float *in, const int32_t *rows, int32_t n_rows, int32_t B, int32_t D, int32_t k,
                               const double *mean, const double *comp, const double *comp_t, const double *std, double sigma,
                               int32_t stages, float *out, int32_t *flag, d3ga_stream_t stream) {
    if (B < 1 || D < 1 || D > D3GA_POSE_MAX_D || k < 1 || k > D3GA_POSE_MAX_D) return D3GA_E_SIZE;
    if (rows && (n_rows < 1 || (int64_t)n_rows * D > INT32_MAX)) return D3GA_E_SIZE;
    if (!pp_stages_valid(stages) || (rows && !(stages & D3GA_POSE_STAGE_PROJECT))) return D3GA_E_CONFIG;
    if (sigma != sigma) return D3GA_E_CONFIG;                // NaN
    if (!in || !mean || !comp || !comp_t || !std || !out || (rows && !flag)) return D3GA_E_NULL;
    if (((uintptr_t)mean | (uintptr_t)comp | (uintptr_t)comp_t | (uintptr_t)std) & 7) return D3GA_E_CONFIG;
    hipStream_t s = (hipStream_t)stream;
    if (rows)
        hipLaunchKernelGGL((pose_clamp_kernel<true>), dim3(B), dim3(kBlock), 0, s, in, rows, n_rows, D, k, mean, comp, comp_t, std, sigma,
                           stages, out, flag);
    else
        hipLaunchKernelGGL((pose_clamp_kernel<false>), dim3(B), dim3(kBlock), 0, s, in, rows, n_rows, D, k, mean, comp, comp_t, std, sigma,
                           stages, out, flag);
    return check_launch(s, 0);
}
