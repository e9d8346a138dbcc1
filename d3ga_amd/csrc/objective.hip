// objective.hip -- the training objective: what turns the per-frame losses and regularisers into the number the
// optimizer sees, and the test that it is a number.
//   scale_energy_*  models/cage_net.py:214, 226: th.mean(th.mean(exp(scaling + delta_scale)**2, axis=1)) without the (P,3)
//                   activated scales ever being written (cage_deform(..., scale_activation="exp") exists so that they are not).
//   objective_*     train.py:190-244: color = (1-l) l1 + l (1-ssim), code_reg, l2_poses, blur_reg, scale_energy * 175,
//                   fm_energy.mean(0) + 3, the five th.stack(...).mean(), the weights and the running `loss +=` -- about a
//                   hundred one-element ATen launches forward and backward -- as ONE launch each way, plus check_loss
//                   (train.py:64-69, a host synchronisation per step) as three status words the forward keeps.
//
// The objective's inputs are a few hundred floats (a few thousand at the limits): what it costs inside a replayed graph is a
// launch, so the forward is one workgroup.  Wavefront w takes entries w, w + 16, ... of the frame-major table; its 64 lanes add
// the entry in the order of objective_math.h; thread 0 then runs obj_assemble -- the text the host tests run -- on the sums.
// The table of pointers and lengths travels in the kernel arguments: inside a captured step the inputs are tensors of the
// graph's private pool, whose addresses differ from the warm-up's, and a table in device memory would have to be filled by a
// copy node inside the graph (see zero_async in d3ga_internal.h for what this stack does with such nodes).
#include "d3ga_internal.h"
#include "objective_math.h"
#include "wave_prims.h"

namespace d3ga {

constexpr int kObjBlock = 1024;                  // 16 wavefronts: the 9 entries of one frame in one round

static_assert(kObjLanes == 64, "obj_lane_partial deals an entry to the lanes that wave_sum adds: a whole wavefront");

// ---- scale_energy ----------------------------------------------------------------------------------------------------------
// One partial per workgroup: a thread adds the four terms of a 16-byte load pairwise, its loads in grid-stride order; 64 lanes
// by butterfly; the four wavefronts in order.
template <int ACT, bool DELTA>
__global__ __launch_bounds__(kBlock) void scale_energy_partial_kernel(int64_t n4, int64_t n, const float *__restrict__ a,
                                                                       const float *__restrict__ b, float *__restrict__ partials) {
    __shared__ float s_part[kBlock / 64];
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    float acc = 0.f;
    for (int64_t i = gid; i < n4; i += stride) {
        float4 x = reinterpret_cast<const float4 *>(a)[i];
        if constexpr (DELTA) {
            const float4 y = reinterpret_cast<const float4 *>(b)[i];
            x.x += y.x; x.y += y.y; x.z += y.z; x.w += y.w;
        }
        acc += (scale_energy_term(ACT, x.x) + scale_energy_term(ACT, x.y)) + (scale_energy_term(ACT, x.z) + scale_energy_term(ACT, x.w));
    }
    for (int64_t i = 4 * n4 + gid; i < n; i += stride) acc += scale_energy_term(ACT, DELTA ? a[i] + b[i] : a[i]);
    wave_sums_to_lds(acc, s_part);
    if (threadIdx.x == 0) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) t += s_part[w];
        partials[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(kBlock) void scale_energy_finish_kernel(int np, const float *__restrict__ partials, float fn,
                                                                      float *__restrict__ out) {
    __shared__ float s_part[kBlock / 64];
    float acc = 0.f;
    for (int i = threadIdx.x; i < np; i += kBlock) acc += partials[i];
    wave_sums_to_lds(acc, s_part);
    if (threadIdx.x == 0) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) t += s_part[w];
        out[0] = t / fn;
    }
}

template <int ACT, bool DELTA>
__global__ __launch_bounds__(kBlock) void scale_energy_bwd_kernel(int64_t n4, int64_t n, const float *__restrict__ a,
                                                                   const float *__restrict__ b, const float *__restrict__ g, float fn,
                                                                   float *__restrict__ grad) {
    const float s = g[0] / fn;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    for (int64_t i = gid; i < n4; i += stride) {
        float4 x = reinterpret_cast<const float4 *>(a)[i];
        if constexpr (DELTA) {
            const float4 y = reinterpret_cast<const float4 *>(b)[i];
            x.x += y.x; x.y += y.y; x.z += y.z; x.w += y.w;
        }
        reinterpret_cast<float4 *>(grad)[i] = make_float4(s * scale_energy_dterm(ACT, x.x), s * scale_energy_dterm(ACT, x.y),
                                                          s * scale_energy_dterm(ACT, x.z), s * scale_energy_dterm(ACT, x.w));
    }
    for (int64_t i = 4 * n4 + gid; i < n; i += stride) grad[i] = s * scale_energy_dterm(ACT, DELTA ? a[i] + b[i] : a[i]);
}

// ---- the assembly ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kObjBlock) void objective_fwd_kernel(d3ga_objective_desc d, float *__restrict__ out,
                                                                   int32_t *__restrict__ status) {
    __shared__ float s_sum[D3GA_OBJ_MAX_FRAMES * D3GA_OBJ_SLOTS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n_items = d.n_frames * D3GA_OBJ_SLOTS;
    for (int it = wave; it < n_items; it += kObjBlock / 64) {
        const d3ga_objective_entry e = d.entry[it];
        float v = 0.f;
        if (e.ptr) v = wave_sum(obj_lane_partial(it % D3GA_OBJ_SLOTS, e.ptr, e.len, lane));
        if (lane == 0) s_sum[it] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float terms[D3GA_OBJ_TERMS];
        obj_assemble(d, s_sum, terms);
        out[0] = terms[kTermTotal];
#pragma unroll
        for (int k = 0; k < D3GA_OBJ_TERMS; ++k) out[1 + k] = terms[k];
        obj_status_update(status, terms);
    }
}

// a thread per element of an entry, the entries one after the other (their loads do not depend on each other)
__global__ __launch_bounds__(kBlock) void objective_bwd_kernel(d3ga_objective_desc d, const float *__restrict__ g,
                                                                float *__restrict__ grads) {
    const float gv = g[0];
    const int n_items = d.n_frames * D3GA_OBJ_SLOTS;
    const int gid = blockIdx.x * kBlock + threadIdx.x, stride = gridDim.x * kBlock;
    for (int it = 0; it < n_items; ++it) {
        const d3ga_objective_entry e = d.entry[it];
        if (!e.ptr || e.goff < 0) continue;
        const int slot = it % D3GA_OBJ_SLOTS;
        const bool reads = slot == kObjEncoding || slot == kObjPoses || slot == kObjBlur;
        for (int i = gid; i < e.len; i += stride) grads[e.goff + i] = obj_grad(d, slot, e.len, reads ? e.ptr[i] : 0.f, gv);
    }
}

}  // namespace d3ga

using namespace d3ga;

static inline int scale_energy_grid(int64_t n4, int cap) {
    const int64_t blocks = (n4 + kBlock - 1) / kBlock;
    return (int)(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
}

extern "C" int d3ga_scale_energy_fwd(int64_t n, const float *scaling, const float *delta, int32_t activation, float *out,
                                     float *partials, d3ga_stream_t stream) {
    if (n <= 0) return D3GA_E_SIZE;
    if (!scaling || !out || !partials) return D3GA_E_NULL;
    if (activation != D3GA_SCALE_ACT_EXP && activation != D3GA_SCALE_ACT_NONE) return D3GA_E_CONFIG;
    if (!aligned16(scaling) || !aligned16(delta)) return D3GA_E_CONFIG;
    static_assert(D3GA_SCALE_ENERGY_GRID <= D3GA_LOSS_PARTIALS, "one partial per workgroup");
    hipStream_t s = (hipStream_t)stream;
    const int64_t n4 = n / 4;
    const int np = scale_energy_grid(n4, D3GA_SCALE_ENERGY_GRID);
    const bool ex = activation == D3GA_SCALE_ACT_EXP;
#define D3GA_SE_FWD(ACT, DELTA) \
    hipLaunchKernelGGL((scale_energy_partial_kernel<ACT, DELTA>), dim3(np), dim3(kBlock), 0, s, n4, n, scaling, delta, partials)
    if (ex && delta) D3GA_SE_FWD(D3GA_SCALE_ACT_EXP, true);
    else if (ex) D3GA_SE_FWD(D3GA_SCALE_ACT_EXP, false);
    else if (delta) D3GA_SE_FWD(D3GA_SCALE_ACT_NONE, true);
    else D3GA_SE_FWD(D3GA_SCALE_ACT_NONE, false);
#undef D3GA_SE_FWD
    hipLaunchKernelGGL(scale_energy_finish_kernel, dim3(1), dim3(kBlock), 0, s, np, (const float *)partials, (float)n, out);
    return check_launch(s, 0);
}

extern "C" int d3ga_scale_energy_bwd(int64_t n, const float *scaling, const float *delta, int32_t activation, const float *g,
                                     float *grad, d3ga_stream_t stream) {
    if (n <= 0) return D3GA_E_SIZE;
    if (!scaling || !g || !grad) return D3GA_E_NULL;
    if (activation != D3GA_SCALE_ACT_EXP && activation != D3GA_SCALE_ACT_NONE) return D3GA_E_CONFIG;
    if (!aligned16(scaling) || !aligned16(delta) || !aligned16(grad)) return D3GA_E_CONFIG;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n4 = n / 4;
    const int nb = scale_energy_grid(n4, 2048);
    const bool ex = activation == D3GA_SCALE_ACT_EXP;
#define D3GA_SE_BWD(ACT, DELTA) \
    hipLaunchKernelGGL((scale_energy_bwd_kernel<ACT, DELTA>), dim3(nb), dim3(kBlock), 0, s, n4, n, scaling, delta, g, (float)n, grad)
    if (ex && delta) D3GA_SE_BWD(D3GA_SCALE_ACT_EXP, true);
    else if (ex) D3GA_SE_BWD(D3GA_SCALE_ACT_EXP, false);
    else if (delta) D3GA_SE_BWD(D3GA_SCALE_ACT_NONE, true);
    else D3GA_SE_BWD(D3GA_SCALE_ACT_NONE, false);
#undef D3GA_SE_BWD
    return check_launch(s, 0);
}

// The caller's table, checked, into `out` with everything the kernels must not look at cleared.  n_grads < 0: the forward
// (offsets are not read); else every entry with goff >= 0 must lie inside [0, n_grads).
static int objective_desc(const d3ga_objective_desc *desc, int64_t n_grads, d3ga_objective_desc *out, int64_t *n_elems) {
    if (!desc) return D3GA_E_NULL;
    if (desc->n_frames < 1 || desc->n_frames > D3GA_OBJ_MAX_FRAMES) return D3GA_E_SIZE;
    *out = *desc;
    out->reserved = 0;
    int64_t elems = 0;
    for (int f = 0; f < D3GA_OBJ_MAX_FRAMES; ++f)
        for (int k = 0; k < D3GA_OBJ_SLOTS; ++k) {
            d3ga_objective_entry &e = out->entry[f * D3GA_OBJ_SLOTS + k];
            if (f >= desc->n_frames || !e.ptr) {
                const bool optional = k == kObjFmEnergy || k == kObjPoses || k == kObjBlur || k == kObjVgg;
                if (f < desc->n_frames && !optional) return D3GA_E_NULL;
                e = d3ga_objective_entry{nullptr, 0, -1};
                continue;
            }
            const bool scalar = k == kObjL1 || k == kObjSsim || k == kObjSilL1 || k == kObjVgg;
            if (e.len < 1 || e.len > (scalar ? 1 : D3GA_OBJ_MAX_LEN)) return D3GA_E_SIZE;
            if (n_grads < 0) e.goff = -1;
            else if (e.goff >= 0) {
                if ((int64_t)e.goff + e.len > n_grads) return D3GA_E_SIZE;
                elems += e.len;
            } else e.goff = -1;
        }
    for (int f = 1; f < desc->n_frames; ++f)
        for (int k = 0; k < D3GA_OBJ_SLOTS; ++k) {
            const d3ga_objective_entry &e = out->entry[f * D3GA_OBJ_SLOTS + k], &e0 = out->entry[k];
            if ((e.ptr == nullptr) != (e0.ptr == nullptr)) return D3GA_E_CONFIG;
            if ((k == kObjScaleEnergy || k == kObjFmEnergy) && e.len != e0.len) return D3GA_E_CONFIG;
        }
    if (n_elems) *n_elems = elems;
    return 0;
}

extern "C" int d3ga_objective_fwd(const d3ga_objective_desc *desc, float *out, int32_t *status, d3ga_stream_t stream) {
    d3ga_objective_desc d;
    D3GA_TRY(objective_desc(desc, -1, &d, nullptr));
    if (!out || !status) return D3GA_E_NULL;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(objective_fwd_kernel, dim3(1), dim3(kObjBlock), 0, s, d, out, status);
    return check_launch(s, 0);
}

extern "C" int d3ga_objective_bwd(const d3ga_objective_desc *desc, const float *g, float *grads, int64_t n_grads,
                                  d3ga_stream_t stream) {
    if (n_grads < 0) return D3GA_E_SIZE;
    d3ga_objective_desc d;
    int64_t elems = 0;
    D3GA_TRY(objective_desc(desc, n_grads, &d, &elems));
    if (!g || !grads) return D3GA_E_NULL;
    if (elems == 0) return D3GA_OK;
    hipStream_t s = (hipStream_t)stream;
    const int64_t blocks = (elems + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(objective_bwd_kernel, dim3((unsigned)(blocks > 64 ? 64 : blocks)), dim3(kBlock), 0, s, d, g, grads);
    return check_launch(s, 0);
}
