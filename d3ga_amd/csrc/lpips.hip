// lpips.hip -- the head of the LPIPS (VGG) metric, the third figure of the reference's errors_<trajectory>.txt
// (recorder/heatmap.py:13, 40: lpips.LPIPS("vgg")(fake, target); test.py:171-174, 200-206).  Forward only: a metric.  The 13
// convolutions and four pools of VGG16 are perceptual.hip's batched entry points (d3ga_vgg_conv3x3_n, d3ga_vgg_maxpool2_fwd_n)
// with fake and target as ONE batch of N = 2 B images per layer; this file holds what is left (lpips_math.h has the formulas):
//
// lp_input_kernel   (N, 3, H, W) -> channels-last (N, H, W, 3) through the scaling layer.  One thread per output element.
//
// lp_tap_kernel     the distance of one feature tap: a, b (B, h, w, C) -> d (B, h, w) and partial sums of it.  A streaming read
//   of 2 h w C floats with a reduction over the C contiguous channels of a pixel.  A pixel belongs to a GROUP of 2^shift
//   consecutive lanes (lp_group_shift: 16 lanes at C = 64, a whole wavefront from C = 256 on), so a wavefront's load
//   instruction covers consecutive addresses; with C % 4 == 0 and 16-byte aligned tensors a lane moves float4.  Every
//   element is read ONCE: a lane keeps its <= 8 values of a and of b in registers between the norm and the difference.  The
//   group sums by xor shuffles below its own width (every lane of the group ends with the same bits), so a pixel's value
//   depends on C alone -- not on where the pixel sits, which image it belongs to, or how many images there are.
//   blockIdx.y is the image; a workgroup strides over its image's pixels, adds its groups' distances (lane, then the 64
//   lanes by shuffles, then the four wavefronts through LDS) and stores ONE partial.  No atomics.
//
// lp_finish_kernel  one workgroup per image adds the image's partials in index order in double, divides by h w and stores
//   the mean into the image's value cell or adds it to what the cell holds (the sum over the five taps): one thread, one
//   plain load and store.  Two stages in a fixed order: image b of a batch is bit for bit the single-pair call, and a graph
//   replay bit for bit the eager call.
//
// BOUNDS: a lane reads channel index c of pixel p only under `p < hw && c < C`; everything else is a register zero.  The
// map and the partial are written under the same `p < hw` / by one thread per workgroup at [image * gridDim.x + blockIdx.x],
// gridDim.x = lp_tap_blocks <= kLpPartials.
#include "d3ga_internal.h"
#include "lpips_math.h"
#include "wave_prims.h"

namespace d3ga {

__global__ __launch_bounds__(kBlock) void lp_input_kernel(int64_t n, int hw, int normalize, const float *__restrict__ img,
                                                          float *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int c = (int)(i % 3);
        const int64_t q = i / 3;
        const int64_t im = q / hw, p = q - im * hw;
        out[i] = lp_input(img[(im * 3 + c) * hw + p], c, normalize);
    }
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void lp_tap_kernel(int hw, int C, int shift, const float *__restrict__ a,
                                                        const float *__restrict__ b, const float *__restrict__ lin,
                                                        float *__restrict__ map, float *__restrict__ partials) {
    constexpr int IT = VEC ? kLpPassesVec : kLpPassesScalar, V = VEC ? 4 : 1;
    __shared__ float s_part[kBlock / 64];
    const int tid = threadIdx.x;
    const int G = 1 << shift, sub = tid & (G - 1), local = tid >> shift, ppb = kBlock >> shift;
    const size_t img = blockIdx.y;
    const float *ai = a + img * (size_t)hw * (size_t)C, *bi = b + img * (size_t)hw * (size_t)C;

    // this lane's channels: pass k covers c0[k] .. c0[k] + V - 1; the weights are the same for every pixel
    float wl[IT][V];
    bool have[IT];
#pragma unroll
    for (int k = 0; k < IT; ++k) {
        const int c0 = (k * G + sub) * V;
        have[k] = c0 < C;                                             // VEC: C % 4 == 0, the whole quad is inside
        if constexpr (VEC) {
            const float4 q = have[k] ? *reinterpret_cast<const float4 *>(lin + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
            wl[k][0] = q.x; wl[k][1] = q.y; wl[k][2] = q.z; wl[k][3] = q.w;
        } else {
            wl[k][0] = have[k] ? lin[c0] : 0.f;
        }
    }

    float acc = 0.f;
    for (int64_t p0 = (int64_t)blockIdx.x * ppb; p0 < hw; p0 += (int64_t)gridDim.x * ppb) {      // uniform over the workgroup
        const int64_t p = p0 + local;
        const bool ok = p < hw;
        float va[IT][V], vb[IT][V];
#pragma unroll
        for (int k = 0; k < IT; ++k) {
            const size_t o = (size_t)(ok ? p : 0) * (size_t)C + (size_t)((k * G + sub) * V);
            if constexpr (VEC) {
                float4 qa = make_float4(0.f, 0.f, 0.f, 0.f), qb = qa;
                if (ok && have[k]) {
                    qa = *reinterpret_cast<const float4 *>(ai + o);
                    qb = *reinterpret_cast<const float4 *>(bi + o);
                }
                va[k][0] = qa.x; va[k][1] = qa.y; va[k][2] = qa.z; va[k][3] = qa.w;
                vb[k][0] = qb.x; vb[k][1] = qb.y; vb[k][2] = qb.z; vb[k][3] = qb.w;
            } else {
                va[k][0] = (ok && have[k]) ? ai[o] : 0.f;
                vb[k][0] = (ok && have[k]) ? bi[o] : 0.f;
            }
        }
        float sa = 0.f, sb = 0.f;
#pragma unroll
        for (int k = 0; k < IT; ++k)
#pragma unroll
            for (int j = 0; j < V; ++j) { sa += va[k][j] * va[k][j]; sb += vb[k][j] * vb[k][j]; }
        for (int off = 1; off < G; off <<= 1) { sa += __shfl_xor(sa, off); sb += __shfl_xor(sb, off); }
        const float na = sqrtf(sa), nb = sqrtf(sb);
        float d = 0.f;
#pragma unroll
        for (int k = 0; k < IT; ++k)
#pragma unroll
            for (int j = 0; j < V; ++j) d += lp_term(va[k][j], vb[k][j], na, nb, wl[k][j]);
        for (int off = 1; off < G; off <<= 1) d += __shfl_xor(d, off);
        if (sub == 0 && ok) {
            if (map) map[img * (size_t)hw + (size_t)p] = d;
            acc += d;
        }
    }
    wave_sums_to_lds(acc, s_part);
    if (tid == 0) partials[img * gridDim.x + blockIdx.x] = ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
}

__global__ __launch_bounds__(kBlock) void lp_finish_kernel(int np, double hw, int accumulate, const float *__restrict__ partials,
                                                           float *__restrict__ value) {
    __shared__ double s_part[kBlock / 64];
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const float *p = partials + b * (size_t)np;
    double s = 0.0;
    for (int i = tid; i < np; i += kBlock) s += (double)p[i];
    wave_sums_to_lds(s, s_part);
    if (tid == 0) {
        const float mean = (float)((((s_part[0] + s_part[1]) + s_part[2]) + s_part[3]) / hw);
        value[b] = accumulate ? value[b] + mean : mean;
    }
}

// every element index of (n, h, w, c) fits an int32
static inline bool lp_sizes_ok(int64_t n, int64_t h, int64_t w, int64_t c) {
    return n > 0 && h > 0 && w > 0 && c > 0 && h * w <= INT32_MAX && n * h * w <= INT32_MAX && n * h * w * c <= INT32_MAX;
}
static inline bool lp_overlap(const void *p, int64_t pbytes, const void *q, int64_t qbytes) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return p && q && a < b + (uintptr_t)qbytes && b < a + (uintptr_t)pbytes;
}

}  // namespace d3ga

using namespace d3ga;

extern "C" int d3ga_lpips_input(int32_t N, int32_t H, int32_t W, int32_t normalize, const float *img, float *out,
                                d3ga_stream_t stream) {
    if (!lp_sizes_ok(N, H, W, 3)) return D3GA_E_SIZE;
    if (!img || !out) return D3GA_E_NULL;
    if (normalize & ~1) return D3GA_E_CONFIG;
    if (((uintptr_t)img | (uintptr_t)out) & 3) return D3GA_E_CONFIG;
    const int64_t n = (int64_t)N * H * W * 3;
    if (lp_overlap(img, 4 * n, out, 4 * n)) return D3GA_E_CONFIG;     // a transpose cannot run in place
    hipStream_t s = (hipStream_t)stream;
    const int64_t blocks = (n + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(lp_input_kernel, dim3((unsigned)(blocks > 65536 ? 65536 : blocks)), dim3(kBlock), 0, s, n, H * W, normalize, img, out);
    return check_launch(s, 0);
}

extern "C" int d3ga_lpips_tap(int32_t B, int32_t h, int32_t w, int32_t C, const float *a, const float *b, const float *lin,
                              float *map, float *partials, float *value, int32_t accumulate, d3ga_stream_t stream) {
    if (!lp_sizes_ok(B, h, w, C) || C > kLpMaxC || B > 65535) return D3GA_E_SIZE;
    if (!a || !b || !lin || !partials || !value) return D3GA_E_NULL;
    if (accumulate & ~1) return D3GA_E_CONFIG;
    if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)lin | (uintptr_t)map | (uintptr_t)partials | (uintptr_t)value) & 3) return D3GA_E_CONFIG;
    const int64_t hw = (int64_t)h * w, in_bytes = 4 * B * hw * C;
    const void *outs[3] = {map, partials, value};
    const int64_t out_bytes[3] = {4 * B * hw, 4 * (int64_t)B * kLpPartials, 4 * (int64_t)B};
    for (int i = 0; i < 3; ++i) {                                      // no output may lie in an input or in another output
        if (lp_overlap(outs[i], out_bytes[i], a, in_bytes) || lp_overlap(outs[i], out_bytes[i], b, in_bytes) ||
            lp_overlap(outs[i], out_bytes[i], lin, 4 * (int64_t)C))
            return D3GA_E_CONFIG;
        for (int j = i + 1; j < 3; ++j)
            if (lp_overlap(outs[i], out_bytes[i], outs[j], out_bytes[j])) return D3GA_E_CONFIG;
    }
    const bool vec = (C & 3) == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)lin) & 15) == 0;
    const int shift = lp_group_shift(C, vec), np = lp_tap_blocks(hw, shift);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)np, (unsigned)B);
    if (vec) hipLaunchKernelGGL((lp_tap_kernel<true>), grid, dim3(kBlock), 0, s, (int)hw, C, shift, a, b, lin, map, partials);
    else hipLaunchKernelGGL((lp_tap_kernel<false>), grid, dim3(kBlock), 0, s, (int)hw, C, shift, a, b, lin, map, partials);
    D3GA_TRY(check_launch(s, 0));
    hipLaunchKernelGGL(lp_finish_kernel, dim3((unsigned)B), dim3(kBlock), 0, s, np, (double)hw, accumulate, partials, value);
    return check_launch(s, 0);
}

extern "C" int d3ga_lpips_scratch_bytes(int32_t B, int32_t H, int32_t W, const int32_t *widths, int64_t *out) {
    if (!out) return D3GA_E_NULL;
    if (B <= 0 || B > 65535 || H < kLpMinSide || W < kLpMinSide) return D3GA_E_SIZE;
    const int64_t n = 2 * (int64_t)B;                                 // fake and target in lockstep: one batch per layer
    int64_t h = H, w = W, biggest = n * h * w * 3;
    if (biggest > INT32_MAX) return D3GA_E_SIZE;
    for (int i = 0; i < kLpConvs; ++i) {
        const int64_t c = widths ? widths[i] : lp_vgg16_width(i);
        if (c <= 0 || (lp_is_tap(i) && c > kLpMaxC)) return D3GA_E_SIZE;
        if (lp_pool_before(i)) { h /= 2; w /= 2; }
        if (n * h * w * c > INT32_MAX) return D3GA_E_SIZE;
        if (n * h * w * c > biggest) biggest = n * h * w * c;
    }
    out[1] = align256(4 * biggest);                                   // one buffer of the ping-pong
    out[2] = align256(4 * (int64_t)B * kLpPartials);                  // the distance's partial sums
    out[0] = 2 * out[1] + out[2];                                     // ping | pong | partials
    return D3GA_OK;
}
