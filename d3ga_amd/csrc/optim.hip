// optim.hip -- gradient clipping + Adam for ALL parameters of a model in three launches (models/trainer.py:186-192:
// clip_grad_norm_(parameters, 2.5) followed by torch.optim.Adam.step()).
//
// The parameters are described by a CHUNK TABLE in device memory (include/d3ga.h: d3ga_optim_chunk): one record per run of at
// most D3GA_OPTIM_CHUNK elements of one tensor.  Every launch walks that table, so the launch count does not depend on the
// number of tensors.
//   1. optim_gradnorm_kernel   sum g^2 per chunk -> partials[chunk]   (a plain store to a fixed slot: no float atomics, the
//                              sum of a chunk depends on the chunk's data alone, not on the grid); it also leaves a copy of
//                              the records it read in the scratch buffer for launch 3, so that a table kept in pinned HOST
//                              memory (a captured step: include/d3ga.h) crosses the bus once per step
//   2. optim_prepare_kernel    one workgroup: partials added in double in a fixed order (thread t takes partials t, t + 256,
//                              ..., then an LDS tree over the 256 threads) -> grad_norm, clip_coef; per tensor
//                              step += 1 and the bias corrections (powers in double) -> tensor_consts[tensor]
//   3. optim_adam_kernel       g' = clip_coef g; m = b1 m + (1 - b1) g'; v = b2 v + (1 - b2) g'^2;
//                              p -= step_size m / (sqrt(v) inv_sqrt_bc2 + eps)
// Traffic of 3: read g, p, m, v, write p, m, v = 7 dwords per element; 1 adds one read of g.  Both are bandwidth-bound:
// sqrt and the division are the IEEE ones.
#include "d3ga_internal.h"
#include "wave_prims.h"

namespace d3ga {

static_assert(sizeof(d3ga_optim_chunk) == 48, "d3ga_optim_chunk layout (include/d3ga.h)");
static_assert(sizeof(d3ga_optim_tensor) == 16, "d3ga_optim_tensor layout (include/d3ga.h)");

// The tensor pointers come out of a table in memory, so the compiler knows no address space for them and would emit flat_*
// accesses (which also wait on the LDS counter).  They are global memory by contract: say so.
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) float gf32;
typedef __attribute__((address_space(1))) const float gcf32;
typedef __attribute__((address_space(1))) f32x4 gf32x4;
typedef __attribute__((address_space(1))) const f32x4 gcf32x4;

constexpr int kOptimGridCap = 2048;          // 256 CUs x 8 workgroups; the table is walked with a grid stride
// workgroups for n_chunks records: at most the cap, and so many that every workgroup makes the same number of trips (3671
// chunks -> 1836 workgroups x 2, not 2048 of which 425 make one trip and leave a fifth of the chip idle behind the rest)
static inline int optim_grid(int n_chunks) {
    const int trips = (n_chunks + kOptimGridCap - 1) / kOptimGridCap;
    return (n_chunks + trips - 1) / trips;
}

// what launch 2 leaves for launch 3, per tensor (32 bytes: one scalar load per chunk)
struct OptimTensorConsts {
    float step_size, inv_sqrt_bc2, beta1, one_minus_beta1, beta2, one_minus_beta2, eps, pad;
};

struct OptimScratch {
    float *partials;              // n_chunks
    float *clip_coef;             // 1 (a 256-byte section)
    OptimTensorConsts *consts;    // n_tensors
    d3ga_optim_chunk *table_copy; // n_chunks
};
static inline int64_t optim_scratch_bytes(int64_t n_chunks, int64_t n_tensors) {
    return align256(4 * n_chunks) + 256 + align256((int64_t)sizeof(OptimTensorConsts) * n_tensors) +
           align256((int64_t)sizeof(d3ga_optim_chunk) * n_chunks);
}
static inline OptimScratch carve_optim(void *base, int64_t n_chunks, int64_t n_tensors) {
    char *p = (char *)base;
    OptimScratch s;
    s.partials = (float *)p;   p += align256(4 * n_chunks);
    s.clip_coef = (float *)p;  p += 256;
    s.consts = (OptimTensorConsts *)p;      p += align256((int64_t)sizeof(OptimTensorConsts) * n_tensors);
    s.table_copy = (d3ga_optim_chunk *)p;
    return s;
}

// sum over the 256 threads of a workgroup, in a fixed order (butterfly inside a wavefront, then the four wavefronts in
// index order); valid in thread 0.  s_red: 4 floats.
__device__ __forceinline__ float block_sum_256(float x, float *s_red) {
    __syncthreads();                                     // the previous chunk's readers are done with s_red
    wave_sums_to_lds(x, s_red);
    return (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

__global__ void __launch_bounds__(256) optim_gradnorm_kernel(const d3ga_optim_chunk *__restrict__ table, int n_chunks,
                                                             float *__restrict__ partials,
                                                             d3ga_optim_chunk *__restrict__ table_copy) {
    __shared__ float s_red[4];
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const d3ga_optim_chunk ch = table[c];
        const int n = min(ch.n, D3GA_OPTIM_CHUNK);
        gcf32 *__restrict__ g = (gcf32 *)ch.g;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        if (ch.flags & D3GA_OPTIM_ALIGNED16) {
            const int n4 = n >> 2;
            gcf32x4 *__restrict__ g4 = (gcf32x4 *)ch.g;
            for (int i = threadIdx.x; i < n4; i += 256) {
                const f32x4 x = g4[i];
                a0 = fmaf(x.x, x.x, a0); a1 = fmaf(x.y, x.y, a1); a2 = fmaf(x.z, x.z, a2); a3 = fmaf(x.w, x.w, a3);
            }
            const int i = (n4 << 2) + threadIdx.x;       // at most 3 elements behind the last whole float4
            if (i < n) { const float x = g[i]; a0 = fmaf(x, x, a0); }
        } else {
            for (int i = threadIdx.x; i < n; i += 256) { const float x = g[i]; a0 = fmaf(x, x, a0); }
        }
        const float s = block_sum_256((a0 + a1) + (a2 + a3), s_red);
        if (threadIdx.x == 0) { partials[c] = s; table_copy[c] = ch; }
    }
}

__global__ void __launch_bounds__(256) optim_prepare_kernel(const float *__restrict__ partials, int n_partials,
                                                            const d3ga_optim_tensor *__restrict__ tensors, int n_tensors,
                                                            const double *__restrict__ hparams, int n_groups, float max_norm,
                                                            float *__restrict__ clip_coef, float *__restrict__ grad_norm_out,
                                                            OptimTensorConsts *__restrict__ consts) {
    __shared__ double s_sum[256];
    if (n_partials > 0) {            // clipping on
        double acc = 0.0;
        for (int i = threadIdx.x; i < n_partials; i += 256) acc += (double)partials[i];
        s_sum[threadIdx.x] = acc;
        __syncthreads();
        for (int w = 128; w >= 1; w >>= 1) {
            if ((int)threadIdx.x < w) s_sum[threadIdx.x] += s_sum[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            const double norm = sqrt(s_sum[0]);
            const double c = (double)max_norm / (norm + 1e-6);
            clip_coef[0] = c > 1.0 ? 1.0f : (float)c;        // (a NaN norm stays a NaN coefficient, as torch's clamp leaves it)
            if (grad_norm_out) grad_norm_out[0] = (float)norm;
        }
    } else if (threadIdx.x == 0) {
        clip_coef[0] = 1.0f;
    }
    for (int t = threadIdx.x; t < n_tensors; t += 256) {
        const d3ga_optim_tensor ts = tensors[t];
        const int grp = min(max(ts.group, 0), n_groups - 1);
        const double lr = hparams[4 * grp], b1 = hparams[4 * grp + 1], b2 = hparams[4 * grp + 2], eps = hparams[4 * grp + 3];
        gf32 *step_cell = (gf32 *)ts.step;
        const float step = step_cell[0] + 1.0f;
        step_cell[0] = step;
        OptimTensorConsts k;
        k.step_size = (float)(lr / (1.0 - pow(b1, (double)step)));
        k.inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow(b2, (double)step)));
        k.beta1 = (float)b1; k.one_minus_beta1 = (float)(1.0 - b1);
        k.beta2 = (float)b2; k.one_minus_beta2 = (float)(1.0 - b2);
        k.eps = (float)eps; k.pad = 0.f;
        consts[t] = k;
    }
}

__device__ __forceinline__ void adam_element(float &p, float g, float &m, float &v, float coef, const OptimTensorConsts &k) {
    g *= coef;
    m = k.beta1 * m + k.one_minus_beta1 * g;
    v = k.beta2 * v + k.one_minus_beta2 * (g * g);
    p -= k.step_size * (m / (sqrtf(v) * k.inv_sqrt_bc2 + k.eps));
}

__global__ void __launch_bounds__(256) optim_adam_kernel(const d3ga_optim_chunk *__restrict__ table, int n_chunks, int n_tensors,
                                                         const float *__restrict__ clip_coef,
                                                         const OptimTensorConsts *__restrict__ consts) {
    const float coef = clip_coef[0];
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const d3ga_optim_chunk ch = table[c];
        const OptimTensorConsts k = consts[min(max(ch.tensor, 0), n_tensors - 1)];
        const int n = min(ch.n, D3GA_OPTIM_CHUNK);
        gf32 *__restrict__ p1 = (gf32 *)ch.p, *__restrict__ m1 = (gf32 *)ch.m, *__restrict__ v1 = (gf32 *)ch.v;
        gcf32 *__restrict__ g1 = (gcf32 *)ch.g;
        if (ch.flags & D3GA_OPTIM_ALIGNED16) {
            const int n4 = n >> 2;
            gf32x4 *__restrict__ p4 = (gf32x4 *)ch.p, *__restrict__ m4 = (gf32x4 *)ch.m, *__restrict__ v4 = (gf32x4 *)ch.v;
            gcf32x4 *__restrict__ g4 = (gcf32x4 *)ch.g;
#pragma unroll 2
            for (int i = threadIdx.x; i < n4; i += 256) {
                f32x4 p = p4[i], m = m4[i], v = v4[i];
                const f32x4 g = g4[i];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float pj = p[j], mj = m[j], vj = v[j];
                    adam_element(pj, g[j], mj, vj, coef, k);
                    p[j] = pj; m[j] = mj; v[j] = vj;
                }
                p4[i] = p; m4[i] = m; v4[i] = v;
            }
            const int i = (n4 << 2) + threadIdx.x;
            if (i < n) {
                float p = p1[i], m = m1[i], v = v1[i];
                adam_element(p, g1[i], m, v, coef, k);
                p1[i] = p; m1[i] = m; v1[i] = v;
            }
        } else {
            for (int i = threadIdx.x; i < n; i += 256) {
                float p = p1[i], m = m1[i], v = v1[i];
                adam_element(p, g1[i], m, v, coef, k);
                p1[i] = p; m1[i] = m; v1[i] = v;
            }
        }
    }
}

}  // namespace d3ga

using namespace d3ga;

extern "C" int d3ga_optim_scratch_bytes(int32_t n_chunks, int32_t n_tensors, int32_t n_groups, int64_t *out) {
    if (!out) return D3GA_E_NULL;
    if (n_chunks < 0 || n_tensors < 0 || n_groups < 0) return D3GA_E_SIZE;
    *out = optim_scratch_bytes(n_chunks, n_tensors);
    return D3GA_OK;
}

extern "C" int d3ga_optim_clip_adam_step(const d3ga_optim_chunk *table, int32_t n_chunks, const d3ga_optim_tensor *tensor_state,
                                         int32_t n_tensors, const double *group_hparams, int32_t n_groups, float max_norm,
                                         void *scratch, float *grad_norm_out, d3ga_stream_t stream) {
    if (!table || !tensor_state || !group_hparams || !scratch) return D3GA_E_NULL;
    if (n_chunks <= 0 || n_tensors <= 0 || n_groups <= 0 || n_tensors > n_chunks) return D3GA_E_SIZE;
    hipStream_t s = (hipStream_t)stream;
    const OptimScratch sc = carve_optim(scratch, n_chunks, n_tensors);
    const bool clip = max_norm >= 0.f;
    const int grid = optim_grid(n_chunks);
    if (clip) hipLaunchKernelGGL(optim_gradnorm_kernel, dim3(grid), dim3(256), 0, s, table, n_chunks, sc.partials, sc.table_copy);
    hipLaunchKernelGGL(optim_prepare_kernel, dim3(1), dim3(256), 0, s, (const float *)sc.partials, clip ? n_chunks : 0, tensor_state,
                       n_tensors, group_hparams, n_groups, max_norm, sc.clip_coef, grad_norm_out, sc.consts);
    hipLaunchKernelGGL(optim_adam_kernel, dim3(grid), dim3(256), 0, s, clip ? (const d3ga_optim_chunk *)sc.table_copy : table, n_chunks, n_tensors, (const float *)sc.clip_coef,
                       (const OptimTensorConsts *)sc.consts);
    return check_launch(s, 0);
}
