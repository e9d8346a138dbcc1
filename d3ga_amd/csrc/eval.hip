// eval.hip -- the per-frame tail of the reference's test.py between trainer.fit and the PNG writers, on the device:
//   test.py:140-141,151   a = alpha[0] (1 - float(boundary_fg));  target = image a + (1 - a) bg
//   test.py:186-187       ground_truth = [image a, a]
//   recorder/heatmap.py:16-61   heat = jet[int(min(||target - pred||_2, 1) 256)] (dist_to_rgb), PSNR (utils/image_utils.py:20-22)
//   test.py:171-174,200-206     the running sums behind errors_<trajectory>.txt
// Three kernels, no atomics on any float32 output and no zero fill:
//
// eval_frames_kernel  one launch for B frames, blockIdx.y the frame.  A workgroup streams `passes` passes of 1024 pixels (four
//   per thread and pass): 7 float planes and the boundary bytes in, 10 planes out, 69 bytes per pixel with everything on.  With
//   H W % 4 == 0 and every tensor 16-byte aligned each plane of each frame starts on a 16-byte boundary and a thread moves
//   float4 / uchar4 quads; otherwise the same pixels are moved one by one (coalesced 4-byte accesses; there is no tail in
//   either form: the quad form only runs when the quads tile the plane).  The 257 x 3 jet colours sit in LDS (3 KB), built
//   from the compile-time byte table of eval_math.h.  The squared error is summed per thread, then across the 64 lanes by
//   xor shuffles, then over the four wavefronts through LDS, and stored as one partial per (frame, channel, workgroup).
//
// eval_ssim_kernel  forward-only SSIM (utils/loss_utils.py:46-86), one workgroup per 16 x 16 tile of one channel of one frame
//   (eval_math.h: eval_ssim_tile), one plainly stored partial per tile.  d3ga_ssim_fwd of loss.hip adds its workgroups' sums
//   with float atomics: on the device two calls on the same images gave up to 13 different bit patterns in 300 calls at
//   1080p (4 at 70 x 131), so an evaluation built on it is not reproducible; this kernel is, and loss.hip stays as it is.
//
// eval_finish_kernel  one workgroup per frame adds its partials in index order (the SSIM tiles' in double), forms the three
//   per-channel PSNRs and their mean, writes metrics[b] = (ssim, psnr) and adds (ssim, psnr, 1) to a float64 accumulator (the only atomics here: B
//   float64 adds per call, so that a frame loop needs no read-back per frame).
//
// Additions a squared error passes through, n: 4 passes in the thread (16 up to a 4K frame, at most 128 for the largest frame
// accepted, 2^26 pixels), 6 shuffle steps, 3 over the wavefronts, then at most 8 per thread of the finishing stage (2048
// partials / 256), 6 and 3 again: n <= 16 + 6 + 3 + 8 + 6 + 3 = 42 up to 4K and n <= 154 in all, far below the 2048 behind
// the 1e-3 dB bar.
#include "d3ga_internal.h"
#include "eval_math.h"
#include "wave_prims.h"

namespace d3ga {

static_assert(kEvalBlock == kBlock, "eval_math.h cuts frames for workgroups of kBlock threads");

__device__ constexpr JetTable d_jet = make_jet_table();
static constexpr JetTable h_jet = make_jet_table();

// VEC: quads (H W % 4 == 0, all tensors 16-byte aligned);  BF32: boundary_fg is float32, else bytes
template <bool VEC, bool BF32>
__global__ __launch_bounds__(kBlock) void eval_frames_kernel(int hw, int passes, int flags, const float *__restrict__ pred,
                                                             const float *__restrict__ image, const float *__restrict__ alpha,
                                                             const void *__restrict__ boundary_fg, float *__restrict__ target_out,
                                                             float *__restrict__ gt_out, float *__restrict__ heat_out,
                                                             float *__restrict__ partials) {
    __shared__ float s_jet[3][kJetBad + 1];
    __shared__ float s_part[3][kBlock / 64];
    const int tid = threadIdx.x;
    const size_t b = blockIdx.y;
    if (heat_out) {
        for (int i = tid; i <= kJetBad; i += kBlock) {
#pragma unroll
            for (int c = 0; c < 3; ++c) s_jet[c][i] = jet_colour(d_jet.v[i][c]);
        }
        __syncthreads();
    }
    const bool composed = (flags & D3GA_EVAL_COMPOSED) != 0;
    const float bg = (flags & D3GA_EVAL_BG_WHITE) ? 1.f : 0.f;
    const size_t n = (size_t)hw;
    const float *p3 = pred + b * 3 * n, *i3 = image + b * 3 * n;
    const float *a1 = composed ? nullptr : alpha + b * ((flags & D3GA_EVAL_ALPHA3) ? 3 : 1) * n;      // channel 0 only
    const float *bf = (composed || !BF32) ? nullptr : static_cast<const float *>(boundary_fg) + b * n;
    const uint8_t *bu = (composed || BF32) ? nullptr : static_cast<const uint8_t *>(boundary_fg) + b * n;
    float *t3 = target_out ? target_out + b * 3 * n : nullptr;
    float *g4 = gt_out ? gt_out + b * 4 * n : nullptr;
    float *h3 = heat_out ? heat_out + b * 3 * n : nullptr;
    const int first = blockIdx.x * passes * kEvalPass;       // < hw <= 2^26
    float acc[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < passes; ++k) {
        const int p0 = first + k * kEvalPass;
        if (p0 >= hw) break;                                 // uniform over the workgroup
        if (VEC) {
            const int i = p0 + 4 * tid;
            if (i < hw) {                                    // hw % 4 == 0: the whole quad is inside
                float pr[3][4], im[3][4], al[4] = {1.f, 1.f, 1.f, 1.f}, bd[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float4 q = *reinterpret_cast<const float4 *>(p3 + c * n + i);
                    const float4 r = *reinterpret_cast<const float4 *>(i3 + c * n + i);
                    pr[c][0] = q.x; pr[c][1] = q.y; pr[c][2] = q.z; pr[c][3] = q.w;
                    im[c][0] = r.x; im[c][1] = r.y; im[c][2] = r.z; im[c][3] = r.w;
                }
                if (!composed) {
                    const float4 q = *reinterpret_cast<const float4 *>(a1 + i);
                    al[0] = q.x; al[1] = q.y; al[2] = q.z; al[3] = q.w;
                    if (BF32) {
                        const float4 r = *reinterpret_cast<const float4 *>(bf + i);
                        bd[0] = r.x; bd[1] = r.y; bd[2] = r.z; bd[3] = r.w;
                    } else {
                        const uchar4 r = *reinterpret_cast<const uchar4 *>(bu + i);
                        bd[0] = r.x; bd[1] = r.y; bd[2] = r.z; bd[3] = r.w;
                    }
                }
                EvalPixel px[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    eval_pixel(composed, bg, pr[0][j], pr[1][j], pr[2][j], im[0][j], im[1][j], im[2][j], al[j], bd[j], &px[j]);
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc[c] += px[j].sq[c];
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if (t3) *reinterpret_cast<float4 *>(t3 + c * n + i) = make_float4(px[0].target[c], px[1].target[c], px[2].target[c], px[3].target[c]);
                    if (h3) *reinterpret_cast<float4 *>(h3 + c * n + i) = make_float4(s_jet[c][px[0].bin], s_jet[c][px[1].bin], s_jet[c][px[2].bin], s_jet[c][px[3].bin]);
                }
                if (g4) {
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        *reinterpret_cast<float4 *>(g4 + c * n + i) = make_float4(px[0].gt[c], px[1].gt[c], px[2].gt[c], px[3].gt[c]);
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = p0 + j * kBlock + tid;
                if (i < hw) {
                    const float al = composed ? 1.f : a1[i];
                    const float bd = composed ? 0.f : (BF32 ? bf[i] : (float)bu[i]);
                    EvalPixel px;
                    eval_pixel(composed, bg, p3[i], p3[n + i], p3[2 * n + i], i3[i], i3[n + i], i3[2 * n + i], al, bd, &px);
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        acc[c] += px.sq[c];
                        if (t3) t3[c * n + i] = px.target[c];
                        if (h3) h3[c * n + i] = s_jet[c][px.bin];
                    }
                    if (g4) {
#pragma unroll
                        for (int c = 0; c < 4; ++c) g4[c * n + i] = px.gt[c];
                    }
                }
            }
        }
    }
    if (partials) {
#pragma unroll
        for (int c = 0; c < 3; ++c) wave_sum_to_lds(acc[c], s_part[c]);
        __syncthreads();
        if (tid < 3) partials[(b * 3 + tid) * gridDim.x + blockIdx.x] = ((s_part[tid][0] + s_part[tid][1]) + s_part[tid][2]) + s_part[tid][3];
    }
}

__global__ __launch_bounds__(kBlock) void eval_ssim_kernel(int H, int W, int tiles_x, const float *__restrict__ pred,
                                                           const float *__restrict__ target, float *__restrict__ partials) {
    __shared__ float s_x[kEvalSsimInputs], s_y[kEvalSsimInputs], s_h[5 * kEvalSsimRows];
    __shared__ float s_part[kBlock / 64];
    const int tid = threadIdx.x, tile = blockIdx.x;
    const size_t plane = (size_t)blockIdx.z * 3 + blockIdx.y;
    const size_t o = plane * (size_t)H * W;
    const int ty0 = (tile / tiles_x) * kEvalSsimTile, tx0 = (tile % tiles_x) * kEvalSsimTile;
    float sum = eval_ssim_tile(s_x, s_y, s_h, pred + o, target + o, H, W, ty0, tx0, tid, kBlock, [] { __syncthreads(); });
    wave_sums_to_lds(sum, s_part);
    if (tid == 0) partials[plane * gridDim.x + tile] = ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
}

__global__ __launch_bounds__(kBlock) void eval_finish_kernel(int np, float hw, const float *__restrict__ partials, int64_t np_ssim,
                                                             const float *__restrict__ ssim_partials, float *__restrict__ metrics,
                                                             float *__restrict__ psnr_channels, double *__restrict__ accum) {
    __shared__ float s_part[3][kBlock / 64];
    __shared__ double s_ssim[kBlock / 64];
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float *p = partials + (b * 3 + c) * np;
        float a = 0.f;
        for (int i = tid; i < np; i += kBlock) a += p[i];
        a = wave_sum(a);
        if ((tid & 63) == 0) s_part[c][tid >> 6] = a;
    }
    if (ssim_partials) {                                     // tiles of the three channels, in index order, in double
        const float *p = ssim_partials + b * np_ssim;
        double a = 0.0;
        for (int64_t i = tid; i < np_ssim; i += kBlock) a += (double)p[i];
        wave_sum_to_lds(a, s_ssim);
    }
    __syncthreads();
    if (tid == 0) {
        double mean = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float sum = ((s_part[c][0] + s_part[c][1]) + s_part[c][2]) + s_part[c][3];
            const double db = eval_psnr_db(sum / hw);
            if (psnr_channels) psnr_channels[b * 3 + c] = (float)db;
            mean += db;
        }
        const float psnr = (float)(mean / 3.0);
        const float s = ssim_partials ? (float)((((s_ssim[0] + s_ssim[1]) + s_ssim[2]) + s_ssim[3]) / (3.0 * (double)hw)) : __builtin_nanf("");
        if (metrics) { metrics[2 * b] = s; metrics[2 * b + 1] = psnr; }
        if (accum) {
            atomicAdd(&accum[0], (double)s);
            atomicAdd(&accum[1], (double)psnr);
            atomicAdd(&accum[2], 1.0);
        }
    }
}

}  // namespace d3ga

using namespace d3ga;

static inline bool eval_size_ok(int32_t B, int32_t H, int32_t W) {
    return B > 0 && H > 0 && W > 0 && B <= 65535 && (int64_t)H * W <= kEvalMaxPixels;
}

extern "C" int64_t d3ga_eval_partials(int32_t H, int32_t W) {
    if (H <= 0 || W <= 0 || (int64_t)H * W > kEvalMaxPixels) return D3GA_E_SIZE;
    return eval_partials((int64_t)H * W);
}

extern "C" int d3ga_eval_jet_table(uint8_t *table) {
    if (!table) return D3GA_E_NULL;
    for (int i = 0; i <= kJetBad; ++i)
        for (int c = 0; c < 3; ++c) table[3 * i + c] = h_jet.v[i][c];
    return D3GA_OK;
}

extern "C" int d3ga_eval_frames(int32_t B, int32_t H, int32_t W, int32_t flags, const float *pred, const float *image,
                                const float *alpha, const void *boundary_fg, float *target_out, float *gt_out, float *heat_out,
                                float *partials, d3ga_stream_t stream) {
    if (!eval_size_ok(B, H, W)) return D3GA_E_SIZE;
    if (flags & ~D3GA_EVAL_ALL) return D3GA_E_CONFIG;
    const bool composed = (flags & D3GA_EVAL_COMPOSED) != 0;
    if (!pred || !image || (!composed && (!alpha || !boundary_fg))) return D3GA_E_NULL;
    if (!target_out && !gt_out && !heat_out && !partials) return D3GA_E_NULL;
    if (composed && (target_out || gt_out)) return D3GA_E_CONFIG;          // nothing to compose
    const bool bf32 = (flags & D3GA_EVAL_BOUNDARY_F32) != 0;
    uintptr_t a = (uintptr_t)pred | (uintptr_t)image | (uintptr_t)target_out | (uintptr_t)gt_out | (uintptr_t)heat_out | (uintptr_t)partials;
    if (!composed) a |= (uintptr_t)alpha | (bf32 ? (uintptr_t)boundary_fg : ((uintptr_t)boundary_fg & 3) << 2);
    if (a & 3) return D3GA_E_CONFIG;                                       // not even element-aligned
    const int hw = H * W;
    const bool vec = (hw % 4 == 0) && !(a & 15);
    const int passes = eval_passes(hw);
    const dim3 grid(eval_partials(hw), B);
    hipStream_t s = (hipStream_t)stream;
#define D3GA_EVAL_LAUNCH(V, F)                                                                                                    \
    hipLaunchKernelGGL((eval_frames_kernel<V, F>), grid, dim3(kBlock), 0, s, hw, passes, flags, pred, image, alpha, boundary_fg, \
                       target_out, gt_out, heat_out, partials)
    if (vec) { if (bf32) D3GA_EVAL_LAUNCH(true, true); else D3GA_EVAL_LAUNCH(true, false); }
    else     { if (bf32) D3GA_EVAL_LAUNCH(false, true); else D3GA_EVAL_LAUNCH(false, false); }
#undef D3GA_EVAL_LAUNCH
    return check_launch(s, 0);
}

extern "C" int64_t d3ga_eval_ssim_partials(int32_t H, int32_t W) {
    if (H <= 0 || W <= 0 || (int64_t)H * W > kEvalMaxPixels) return D3GA_E_SIZE;
    return 3 * eval_ssim_tiles(H, W);
}

extern "C" int d3ga_eval_ssim(int32_t B, int32_t H, int32_t W, const float *pred, const float *target, float *ssim_partials,
                              d3ga_stream_t stream) {
    if (!eval_size_ok(B, H, W)) return D3GA_E_SIZE;
    if (!pred || !target || !ssim_partials) return D3GA_E_NULL;
    if (((uintptr_t)pred | (uintptr_t)target | (uintptr_t)ssim_partials) & 3) return D3GA_E_CONFIG;
    hipStream_t s = (hipStream_t)stream;
    const int tiles_x = (W + kEvalSsimTile - 1) / kEvalSsimTile;
    hipLaunchKernelGGL(eval_ssim_kernel, dim3((unsigned)eval_ssim_tiles(H, W), 3, B), dim3(kBlock), 0, s, H, W, tiles_x, pred, target,
                       ssim_partials);
    return check_launch(s, 0);
}

extern "C" int d3ga_eval_finish(int32_t B, int32_t H, int32_t W, const float *partials, const float *ssim_partials, float *metrics,
                                float *psnr_channels, double *accum, d3ga_stream_t stream) {
    if (!eval_size_ok(B, H, W)) return D3GA_E_SIZE;
    if (!partials) return D3GA_E_NULL;
    if (!metrics && !psnr_channels && !accum) return D3GA_E_NULL;
    if (accum && !ssim_partials) return D3GA_E_CONFIG;                     // the running sums carry both metrics
    if ((((uintptr_t)partials | (uintptr_t)ssim_partials | (uintptr_t)metrics | (uintptr_t)psnr_channels) & 3) || ((uintptr_t)accum & 7))
        return D3GA_E_CONFIG;
    hipStream_t s = (hipStream_t)stream;
    const int hw = H * W;
    hipLaunchKernelGGL(eval_finish_kernel, dim3(B), dim3(kBlock), 0, s, eval_partials(hw), (float)hw, partials,
                       (int64_t)(3 * eval_ssim_tiles(H, W)), ssim_partials, metrics, psnr_channels, accum);
    return check_launch(s, 0);
}
