// frame_state.hip -- per-frame state addressed by a DEVICE index, so that a captured training step follows the frame of every
// replay: the latent frame codes and the refined SMPL-X parameters of the reference's GarmentNet.
//   code_lookup_*  models/embeddings.py:13-36 Embedding.forward: nn.Embedding(max_norm) -- torch's embedding_renorm_ on the
//                  looked-up rows IN PLACE, then the row copy -- and the dense weight gradient of its backward.
//   table_mean     Embedding.average(): weight.mean(0, keepdims=True).
//   row_cache_*    models/garment_net.py:87-107, 211-235: three nn.ParameterDict of one (1,D) parameter per frame.  Here a table
//                  (N,D) per dictionary and ONE staged row that the optimizer sees; select writes the staged row back and
//                  stages another one, for the parameter and its Adam moments and step count alike.
//
// These kernels move a few hundred bytes (or one small table): what they cost inside a replayed graph is their launch, so
// every operation is ONE launch of few workgroups (the mean: two, its second stage needs the first one's partial sums).
// Nothing here uses an atomic; every sum has a fixed order, so results are reproducible bit for bit.
//
// Lookup forward: one workgroup.  Thread t holds elements t, t + 256, ... of the row (D <= 4096: at most 16 registers), so a
// row is read once: sum of squares (per thread in element order, 64 lanes by butterfly, the four wavefronts in order), the
// square root, torch's test `norm > max_norm` and scale `max_norm / (norm + 1e-7)`, the store back into the table when the row
// was scaled, and the store into EVERY out row that names this table row.  A table row is handled at its first position in
// idx and skipped at the later ones: renormed once, all copies equal, nothing that was written is read again.
#include "d3ga_internal.h"
#include "wave_prims.h"

namespace d3ga {

constexpr int kCodeRegs = D3GA_CODE_MAX_D / kBlock;          // row elements per thread of the lookup forward
constexpr int kMeanChunks = D3GA_TABLE_MEAN_CHUNKS;          // row chunks (= rows of partial sums) of the mean, at most

__device__ __forceinline__ int code_row(const int32_t *__restrict__ idx, int b, int N) { return min(max(idx[b], 0), N - 1); }

__global__ __launch_bounds__(kBlock) void code_lookup_fwd_kernel(float *__restrict__ table, const int32_t *__restrict__ idx,
                                                                  int N, int D, int B, float max_norm, float *__restrict__ out) {
    __shared__ int s_row[D3GA_CODE_MAX_B];
    __shared__ float s_part[kBlock / 64];
    const int tid = threadIdx.x;
    if (tid < B) s_row[tid] = code_row(idx, tid, N);
    __syncthreads();
    for (int b = 0; b < B; ++b) {
        const int r = s_row[b];
        bool first = true;                                   // (uniform over the workgroup)
        for (int a = 0; a < b; ++a) first = first && s_row[a] != r;
        if (!first) continue;
        float *row = table + (size_t)r * D;
        float v[kCodeRegs];
        float ss = 0.f;
#pragma unroll
        for (int j = 0; j < kCodeRegs; ++j) {
            const int d = tid + j * kBlock;
            v[j] = d < D ? row[d] : 0.f;
            ss = fmaf(v[j], v[j], ss);
        }
        float scale = 1.f;
        bool scaled = false;
        if (max_norm > 0.f) {
            __syncthreads();                                 // the previous row's reads of s_part are done
            wave_sums_to_lds(ss, s_part);
            const float norm = sqrtf(((s_part[0] + s_part[1]) + s_part[2]) + s_part[3]);
            scaled = norm > max_norm;
            if (scaled) scale = max_norm / (norm + 1e-7f);
        }
#pragma unroll
        for (int j = 0; j < kCodeRegs; ++j) {
            const int d = tid + j * kBlock;
            if (d >= D) continue;
            const float x = scaled ? v[j] * scale : v[j];
            if (scaled) row[d] = x;
            for (int c = b; c < B; ++c)
                if (s_row[c] == r) out[(size_t)c * D + d] = x;
        }
    }
}

// dtable[r][d] = sum over the b with idx[b] = r, in increasing b, of dout[b][d]; zero for a row nobody names.  VEC: four
// elements of one row per thread (D % 4 == 0, both tensors 16-byte aligned); else one.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void code_lookup_bwd_kernel(const float *__restrict__ dout, const int32_t *__restrict__ idx,
                                                                  int N, int D, int B, float *__restrict__ dtable) {
    __shared__ int s_row[D3GA_CODE_MAX_B];
    if (threadIdx.x < B) s_row[threadIdx.x] = code_row(idx, threadIdx.x, N);
    __syncthreads();
    constexpr int W = VEC ? 4 : 1;
    const int64_t n = (int64_t)N * D / W;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int64_t e = i * W;
        const int r = (int)(e / D);
        const int d = (int)(e - (int64_t)r * D);
        if constexpr (VEC) {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int b = 0; b < B; ++b) {
                if (s_row[b] != r) continue;
                const float4 q = *reinterpret_cast<const float4 *>(dout + (size_t)b * D + d);
                acc.x += q.x; acc.y += q.y; acc.z += q.z; acc.w += q.w;
            }
            *reinterpret_cast<float4 *>(dtable + e) = acc;
        } else {
            float acc = 0.f;
            for (int b = 0; b < B; ++b)
                if (s_row[b] == r) acc += dout[(size_t)b * D + d];
            dtable[e] = acc;
        }
    }
}

// Mean over the rows, two stages, sums in float64 (the table's mean is a cancelling sum of N zero-mean codes: a float32
// accumulator would leave eps sqrt(N) |x| on a result of |x| / sqrt(N)).  A workgroup is `groups` row groups x `cw` columns
// (cw: a power of two, groups * cw = 256): thread (g, c) adds rows r0 + g, r0 + g + groups, ... of chunk blockIdx.y in row
// order, thread (0, c) adds the groups in order -> partial[chunk][column].  Stage two adds the chunks in order and divides.
__global__ __launch_bounds__(kBlock) void table_mean_partial_kernel(const float *__restrict__ table, int N, int D, int cw,
                                                                     int rows_per_chunk, double *__restrict__ partial) {
    __shared__ double s_sum[kBlock];
    const int tid = threadIdx.x;
    const int c = tid & (cw - 1), g = tid / cw, groups = kBlock / cw;
    const int col = blockIdx.x * cw + c;
    const int r0 = blockIdx.y * rows_per_chunk, r1 = min(r0 + rows_per_chunk, N);
    double acc = 0.0;
    if (col < D)
        for (int r = r0 + g; r < r1; r += groups) acc += (double)table[(size_t)r * D + col];
    s_sum[tid] = acc;
    __syncthreads();
    if (g == 0 && col < D) {
        double s = s_sum[c];
        for (int k = 1; k < groups; ++k) s += s_sum[k * cw + c];
        partial[(size_t)blockIdx.y * D + col] = s;
    }
}

__global__ __launch_bounds__(kBlock) void table_mean_finish_kernel(const double *__restrict__ partial, int N, int D, int chunks,
                                                                    float *__restrict__ out) {
    const int col = blockIdx.x * kBlock + threadIdx.x;
    if (col >= D) return;
    double s = partial[col];
    for (int k = 1; k < chunks; ++k) s += partial[(size_t)k * D + col];
    out[col] = (float)(s / (double)N);
}

struct RowPairs {
    d3ga_row_pair pair[D3GA_ROW_CACHE_MAX_PAIRS];
};

// One workgroup.  SELECT: see include/d3ga.h.  Every thread reads the cells before the barrier, thread 0 writes `prev` behind
// it.  With idx != prev the row written back and the row staged are different rows, and a thread touches element e of both
// and of the stage only: no thread reads what another one writes.
template <bool SELECT>
__global__ __launch_bounds__(kBlock) void row_cache_kernel(RowPairs desc, int n_pairs, const int32_t *__restrict__ idx,
                                                            int32_t *__restrict__ prev, int32_t *__restrict__ flag) {
    const int tid = threadIdx.x;
    const int p = prev[0];
    const int i = SELECT ? idx[0] : p;
    __syncthreads();
    bool ok = true;                                          // (uniform)
    int total = 0;                                           // words of all stages together (12 pairs of actor02: 295)
    for (int k = 0; k < n_pairs; ++k) {
        const int n = desc.pair[k].n_rows;
        ok = ok && p >= -1 && p < n && (!SELECT || (i >= 0 && i < n));
        total += desc.pair[k].width;
    }
    if (!ok) {
        if (tid == 0) flag[0] = 1;
        return;
    }
    if (SELECT && i == p) return;
    // the pairs side by side, a thread per word: both loads of every word are in flight before the first store (a loop over
    // the pairs would be a chain of 2 n_pairs dependent round trips -- the cost of this kernel is latency, not bytes)
    for (int f = tid; f < total; f += kBlock) {
        int k = 0, e = f;
        while (e >= desc.pair[k].width) e -= desc.pair[k++].width;
        const d3ga_row_pair q = desc.pair[k];
        float back = 0.f, row = 0.f;
        if (p >= 0) back = q.stage[e];
        if (SELECT) row = q.table[(size_t)i * q.width + e];
        if (p >= 0) q.table[(size_t)p * q.width + e] = back;
        if (SELECT) q.stage[e] = row;
    }
    if (SELECT && tid == 0) prev[0] = i;
}

}  // namespace d3ga

using namespace d3ga;

static inline int code_shape(int32_t N, int32_t D, int32_t B) {
    if (N < 1 || D < 1 || B < 1 || B > D3GA_CODE_MAX_B || D > D3GA_CODE_MAX_D) return D3GA_E_SIZE;
    if ((int64_t)N * D > INT32_MAX) return D3GA_E_SIZE;
    return 0;
}

extern "C" int d3ga_code_lookup_fwd(float *table, const int32_t *idx, int32_t N, int32_t D, int32_t B, float max_norm,
                                    float *out, d3ga_stream_t stream) {
    D3GA_TRY(code_shape(N, D, B));
    if (!table || !idx || !out) return D3GA_E_NULL;
    if (max_norm != max_norm) return D3GA_E_CONFIG;          // NaN
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(code_lookup_fwd_kernel, dim3(1), dim3(kBlock), 0, s, table, idx, N, D, B, max_norm, out);
    return check_launch(s, 0);
}

extern "C" int d3ga_code_lookup_bwd(const float *dout, const int32_t *idx, int32_t N, int32_t D, int32_t B, float *dtable,
                                    d3ga_stream_t stream) {
    D3GA_TRY(code_shape(N, D, B));
    if (!dout || !idx || !dtable) return D3GA_E_NULL;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = D % 4 == 0 && aligned16(dout) && aligned16(dtable);
    const int64_t n = (int64_t)N * D / (vec ? 4 : 1);
    const int64_t blocks = (n + kBlock - 1) / kBlock;
    const dim3 grid((unsigned)(blocks > 4096 ? 4096 : blocks));
    if (vec) hipLaunchKernelGGL((code_lookup_bwd_kernel<true>), grid, dim3(kBlock), 0, s, dout, idx, N, D, B, dtable);
    else hipLaunchKernelGGL((code_lookup_bwd_kernel<false>), grid, dim3(kBlock), 0, s, dout, idx, N, D, B, dtable);
    return check_launch(s, 0);
}

// column tile (a power of two <= 256), rows per chunk and chunks of the mean's first stage
static inline void mean_plan(int N, int D, int *cw, int *rows_per_chunk, int *chunks) {
    int w = 1;
    while (w < D && w < kBlock) w <<= 1;
    const int groups = kBlock / w;
    int c = (N + 4 * groups - 1) / (4 * groups);             // about four rows per thread ...
    c = c < 1 ? 1 : (c > kMeanChunks ? kMeanChunks : c);     // ... in at most kMeanChunks chunks
    *cw = w;
    *rows_per_chunk = (N + c - 1) / c;
    *chunks = (N + *rows_per_chunk - 1) / *rows_per_chunk;
}

extern "C" int d3ga_table_mean_scratch_bytes(int32_t N, int32_t D, int64_t *bytes) {
    if (!bytes) return D3GA_E_NULL;
    if (N < 1 || D < 1 || (int64_t)N * D > INT32_MAX) return D3GA_E_SIZE;
    *bytes = (int64_t)kMeanChunks * D * (int64_t)sizeof(double);
    return D3GA_OK;
}

extern "C" int d3ga_table_mean(const float *table, int32_t N, int32_t D, float *out, void *scratch, d3ga_stream_t stream) {
    if (N < 1 || D < 1 || (int64_t)N * D > INT32_MAX) return D3GA_E_SIZE;
    if (!table || !out || !scratch) return D3GA_E_NULL;
    if ((uintptr_t)scratch & 7) return D3GA_E_CONFIG;
    int cw, rows_per_chunk, chunks;
    mean_plan(N, D, &cw, &rows_per_chunk, &chunks);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(table_mean_partial_kernel, dim3((D + cw - 1) / cw, chunks), dim3(kBlock), 0, s, table, N, D, cw,
                       rows_per_chunk, (double *)scratch);
    hipLaunchKernelGGL(table_mean_finish_kernel, dim3((D + kBlock - 1) / kBlock), dim3(kBlock), 0, s, (const double *)scratch, N, D,
                       chunks, out);
    return check_launch(s, 0);
}

static inline int row_pairs(const d3ga_row_pair *desc, int32_t n_pairs, RowPairs *out) {
    if (!desc) return D3GA_E_NULL;
    if (n_pairs < 1 || n_pairs > D3GA_ROW_CACHE_MAX_PAIRS) return D3GA_E_SIZE;
    int64_t words = 0;
    for (int k = 0; k < n_pairs; ++k) {
        if (!desc[k].table || !desc[k].stage) return D3GA_E_NULL;
        if (desc[k].width < 1 || desc[k].n_rows < 1 || (int64_t)desc[k].width * desc[k].n_rows > INT32_MAX) return D3GA_E_SIZE;
        words += desc[k].width;
        out->pair[k] = desc[k];
    }
    if (words > INT32_MAX) return D3GA_E_SIZE;
    for (int k = n_pairs; k < D3GA_ROW_CACHE_MAX_PAIRS; ++k) out->pair[k] = d3ga_row_pair{nullptr, nullptr, 0, 0};
    return 0;
}

extern "C" int d3ga_row_cache_select(const d3ga_row_pair *desc, int32_t n_pairs, const int32_t *idx, int32_t *prev,
                                     int32_t *flag, d3ga_stream_t stream) {
    RowPairs rp;
    D3GA_TRY(row_pairs(desc, n_pairs, &rp));
    if (!idx || !prev || !flag) return D3GA_E_NULL;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL((row_cache_kernel<true>), dim3(1), dim3(kBlock), 0, s, rp, n_pairs, idx, prev, flag);
    return check_launch(s, 0);
}

extern "C" int d3ga_row_cache_flush(const d3ga_row_pair *desc, int32_t n_pairs, int32_t *prev, int32_t *flag,
                                    d3ga_stream_t stream) {
    RowPairs rp;
    D3GA_TRY(row_pairs(desc, n_pairs, &rp));
    if (!prev || !flag) return D3GA_E_NULL;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL((row_cache_kernel<false>), dim3(1), dim3(kBlock), 0, s, rp, n_pairs, (const int32_t *)nullptr, prev, flag);
    return check_launch(s, 0);
}
