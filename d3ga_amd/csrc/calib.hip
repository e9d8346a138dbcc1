// calib.hip -- per-camera colour calibration and pixel bias of the Goliath configuration (configs/goliath_axe184.yml:
// use_color_calib, use_pixel_cal).
//   color_calib_*  lib/calibration.py:39-56 (called at models/garment_net.py:265-266): out = rgb * w + b per channel with
//                  (w, b) = corrections[cam][:3], [3:]; the identity camera's colours pass through unchanged.
//   pixel_bias_*   models/color_calib.py:245-258 (added at models/trainer.py:128-131): bias[cam] (1,bh,bw) upsampled
//                  bilinearly to (H,W), F.interpolate's align_corners=False rule, alone or added to an image.
//
// Colour calibration.  The data is cut into SEGMENTS of L consecutive floats whose channel pattern is known: one view of the
// interleaved layout (k,P,3) (L = 3P, element e is channel e % 3) or one plane of the planar layout (k,3,N) (L = N, one
// channel).  blockIdx.y is the segment.  A segment starts h = (-s L) mod 4 floats before a 16-byte boundary (the tensors
// themselves are 16-byte aligned): those h floats and the < 4 floats behind the last whole float4 are done by six threads of
// the segment's first workgroup, everything between by 16-byte accesses, lane t of a workgroup at float4 t, t + 256, t + 512
// of a 768-float4 tile (every wave instruction covers 1 KiB contiguously).  768 is a multiple of 3, so the channel of
// element i of a thread's j-th float4 is (h + t + j + i) % 3 on every trip: the thread rotates (w, b) once by (h + t) % 3
// and indexes the rotated copies with compile-time constants; its six sums are kept in the same rotated frame and turned back
// once.  HBM traffic per Gaussian and view: forward 24 B, backward 36 B (24 B without dL/drgb).
//
// The six sums per view (three of g rgb, three of g) leave each workgroup as one row of six floats in `partials` (plain
// stores); ONE finishing workgroup adds a view's rows in index order, scales, adds the views of a camera in view order and
// writes the whole (n_cameras, 6) gradient -- no atomics, no zero fill, bit-identical from run to run.
//
// Pixel bias backward.  dL/dbias[cam] = U_h^T (sum_c g_c) U_w with U the per-axis interpolation matrices.  Row y of U has at
// most two entries, at i0(y) and i1(y) = min(i0 + 1, n_in - 1), and i0 is non-decreasing in y, so the pixels that touch
// cell i are the contiguous range {y : i - 1 <= i0(y) <= i}.  A workgroup owns 32 cells of one low-resolution row: lane =
// one image column of the cells' x range, summing its column over the row's y range and the channels with the U_h weights
// (coalesced reads) into LDS; then one thread per cell adds its x range with the U_w weights.  Fixed order, no atomics.  The
// same threads write exact zeros into their cells of every OTHER camera's map, so the whole (n_cameras,1,bh,bw) gradient is
// written by the one launch.
#include "d3ga_internal.h"
#include "wave_prims.h"

namespace d3ga {

constexpr int kCalibTile = 3 * kBlock;                       // float4s per workgroup and trip
constexpr int kCalibRows = D3GA_CALIB_PARTIALS / 6;          // rows of six partial sums in the scratch
constexpr int kBiasCells = 32;                               // low-resolution cells per workgroup of the bias backward

__device__ __forceinline__ int calib_cam(const int32_t *__restrict__ cam, int v, int n_cameras) {
    return min(max(cam[v], 0), n_cameras - 1);
}

// BWD = false: dst = out = x w + b (identity: x).
// BWD = true:  src = dL/dout, dst = dL/drgb = g w (identity: g; NULL: skipped); with partials != NULL the six sums of this
//              workgroup go to row (segment * gridDim.x + blockIdx.x) of partials, in the slots of the segment's channels
//              (a planar segment leaves zeros in the other four).  An identity segment writes no row: nobody reads it.
template <bool BWD, bool PLANAR>
__global__ __launch_bounds__(kBlock) void color_calib_kernel(int L, int n_cameras, int identity_idx,
                                                             const float *__restrict__ src, const float *__restrict__ rgb,
                                                             const float *__restrict__ corrections,
                                                             const int32_t *__restrict__ cam, float *__restrict__ dst,
                                                             float *__restrict__ partials) {
#pragma clang fp contract(off)                               // x * w rounded, then + b rounded: the two ATen kernels of the reference
    __shared__ float s_part[6][kBlock / 64];
    const int tid = threadIdx.x;
    const int seg = blockIdx.y;
    const int view = PLANAR ? seg / 3 : seg;
    const int plane = PLANAR ? seg - 3 * view : 0;
    const int c = calib_cam(cam, view, n_cameras);
    const bool ident = c == identity_idx;
    if (BWD && ident && !dst) return;
    const bool sums = BWD && partials && !ident;
    const size_t base = (size_t)seg * (size_t)L;
    const int h = min((int)((4 - (base & 3)) & 3), L);       // floats in front of the first 16-byte boundary
    const int nf = (L - h) >> 2;                             // whole float4s behind them
    const int rot = PLANAR ? 0 : (h + tid) % 3;
    float w[3], b[3];                                        // rotated: element i of float4 j takes w[(j + i) % 3]
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const int ch = PLANAR ? plane : (rot + m) % 3;
        w[m] = corrections[6 * c + ch];
        b[m] = corrections[6 * c + 3 + ch];
    }
    float ax[3] = {0.f, 0.f, 0.f}, ag[3] = {0.f, 0.f, 0.f};  // sums of g x and of g, rotated frame
    const float4 *s4 = reinterpret_cast<const float4 *>(src + base + h);
    const float4 *x4 = reinterpret_cast<const float4 *>((BWD ? rgb : src) + base + h);
    float4 *d4 = reinterpret_cast<float4 *>(dst + base + h);
    for (int f0 = blockIdx.x * kCalibTile; f0 < nf; f0 += gridDim.x * kCalibTile) {
        float4 vs[3], vx[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int f = f0 + j * kBlock + tid;
            if (f < nf) {
                vs[j] = s4[f];
                if (sums) vx[j] = x4[f];
            }
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int f = f0 + j * kBlock + tid;
            if (f >= nf) continue;
            float e[4] = {vs[j].x, vs[j].y, vs[j].z, vs[j].w};
            if (sums) {
                const float x[4] = {vx[j].x, vx[j].y, vx[j].z, vx[j].w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    ax[(j + i) % 3] = fmaf(e[i], x[i], ax[(j + i) % 3]);
                    ag[(j + i) % 3] += e[i];
                }
            }
            if (dst) {
                if (!ident) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) e[i] = BWD ? e[i] * w[(j + i) % 3] : e[i] * w[(j + i) % 3] + b[(j + i) % 3];
                }
                d4[f] = make_float4(e[0], e[1], e[2], e[3]);
            }
        }
    }
    // back to the channel frame: channel ch was slot (ch - rot) mod 3
    float tx[3], tg[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        tx[ch] = rot == 0 ? ax[ch] : rot == 1 ? ax[(ch + 2) % 3] : ax[(ch + 1) % 3];
        tg[ch] = rot == 0 ? ag[ch] : rot == 1 ? ag[(ch + 2) % 3] : ag[(ch + 1) % 3];
    }
    if (PLANAR) {                                            // one channel: the three slots are one sum
        const float sx = (ax[0] + ax[1]) + ax[2], sg = (ag[0] + ag[1]) + ag[2];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) { tx[ch] = ch == plane ? sx : 0.f; tg[ch] = ch == plane ? sg : 0.f; }
    }
    // the h floats in front and the (L - h) % 4 behind: threads 0..5 of the segment's first workgroup, one float each
    if (blockIdx.x == 0 && tid < 6) {
        const int e = tid < 3 ? tid : h + 4 * nf + (tid - 3);
        if (tid < 3 ? e < h : e < L) {
            const int ch = PLANAR ? plane : e % 3;
            const float wc = corrections[6 * c + ch], bc = corrections[6 * c + 3 + ch];
            const float v = src[base + e];
            if (sums) {
                const float x = rgb[base + e];
#pragma unroll
                for (int m = 0; m < 3; ++m)
                    if (m == ch) { tx[m] = fmaf(v, x, tx[m]); tg[m] += v; }
            }
            if (dst) dst[base + e] = ident ? v : (BWD ? v * wc : v * wc + bc);
        }
    }
    if (sums) {                                              // one row per workgroup: plain stores, fixed order
        float r[6] = {tx[0], tx[1], tx[2], tg[0], tg[1], tg[2]};
#pragma unroll
        for (int m = 0; m < 6; ++m) wave_sum_to_lds(r[m], s_part[m]);
        __syncthreads();
        if (tid < 6)
            partials[6 * ((size_t)seg * gridDim.x + blockIdx.x) + tid] =
                (s_part[tid][0] + s_part[tid][1]) + (s_part[tid][2] + s_part[tid][3]);
    }
}

// finishing stage: ONE workgroup.  Zeros the whole (n_cameras, 6) gradient, then view by view adds the view's `rows` rows of
// partials in index order, scales and adds the result to the camera's row (thread 0, so views that share a camera are added
// in view order).  The identity camera's views are skipped: its row stays zero.
__global__ __launch_bounds__(kBlock) void color_calib_finish_kernel(int k, int rows, int n_cameras, int identity_idx,
                                                                    float grad_scale, const float *__restrict__ partials,
                                                                    const int32_t *__restrict__ cam,
                                                                    float *__restrict__ grad_corrections) {
    __shared__ float s_part[6][kBlock / 64];
    const int tid = threadIdx.x;
    for (int i = tid; i < 6 * n_cameras; i += kBlock) grad_corrections[i] = 0.f;
    __syncthreads();
    for (int v = 0; v < k; ++v) {
        const int c = calib_cam(cam, v, n_cameras);
        if (c == identity_idx) continue;                     // (uniform over the workgroup)
        float a[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const float *p = partials + 6 * (size_t)v * rows;
        for (int i = tid; i < rows; i += kBlock) {
#pragma unroll
            for (int m = 0; m < 6; ++m) a[m] += p[6 * i + m];
        }
#pragma unroll
        for (int m = 0; m < 6; ++m) wave_sum_to_lds(a[m], s_part[m]);
        __syncthreads();
        if (tid < 6) {
            const float s = (s_part[tid][0] + s_part[tid][1]) + (s_part[tid][2] + s_part[tid][3]);
            grad_corrections[6 * c + tid] += s * grad_scale;
        }
        __syncthreads();
    }
}

// F.interpolate(mode='bilinear', align_corners=False) along one axis:
//   src = max(0, (dst + 0.5) n_in / n_out - 0.5),  i0 = floor(src),  i1 = min(i0 + 1, n_in - 1),  lambda = src - i0.
// src = ((2 dst + 1) n_in - n_out) / (2 n_out) is a ratio of integers (n_in n_out < 2^30, checked by the entry points), so i0
// is exact and lambda is one rounded quotient -- ATen forms src in float32, 2 eps src away from this; at the Goliath size that
// is 1e-5 of a cell, which a cell's gradient sum would carry as an absolute error
__device__ __forceinline__ void bias_axis(int dst, int n_in, int n_out, int &i0, int &i1, float &lam) {
    const int num = (2 * dst + 1) * n_in - n_out, den = 2 * n_out;
    i0 = num > 0 ? num / den : 0;
    lam = num > 0 ? (float)(num - i0 * den) / (float)den : 0.f;
    i1 = min(i0 + 1, n_in - 1);
}

// first dst in [0, n_out] with i0(dst) >= t (i0 is non-decreasing): (2 dst + 1) n_in >= (2 t + 1) n_out
__device__ __forceinline__ int bias_first(int t, int n_in, int n_out) {
    if (t <= 0) return 0;
    if (t > n_in - 1) return n_out;
    const int c = ((2 * t + 1) * n_out + n_in - 1) / n_in;   // smallest odd-or-even 2 dst + 1 that satisfies it ...
    return c / 2;                                            // ... and the smallest dst with 2 dst + 1 >= c
}

// weight of low-resolution cell i in the interpolation of dst
__device__ __forceinline__ float bias_weight(int dst, int i, int n_in, int n_out) {
    int i0, i1;
    float lam;
    bias_axis(dst, n_in, n_out, i0, i1, lam);
    return (i0 == i ? 1.f - lam : 0.f) + (i1 == i ? lam : 0.f);
}

// out[c] = (image ? image[c] : 0) + up(bias[cam]); a workgroup (64 x 4 threads) owns a 64 x 16 pixel tile
__global__ __launch_bounds__(kBlock) void pixel_bias_fwd_kernel(int C, int H, int W, int n_cameras, int bh, int bw,
                                                                const float *__restrict__ bias,
                                                                const int32_t *__restrict__ cam,
                                                                const float *__restrict__ image, float *__restrict__ out) {
#pragma clang fp contract(off)
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    if (x >= W) return;
    const float *map = bias + (size_t)calib_cam(cam, 0, n_cameras) * bh * bw;
    int x0, x1;
    float lx;
    bias_axis(x, bw, W, x0, x1, lx);
    const size_t hw = (size_t)H * W;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int y = blockIdx.y * 16 + 4 * r + (threadIdx.x >> 6);
        if (y >= H) continue;
        int y0, y1;
        float ly;
        bias_axis(y, bh, H, y0, y1, ly);
        // a + lambda (b - a): exact on a constant map, error ~ eps |a| + 2 eps |b - a| per blend
        const float v00 = map[(size_t)y0 * bw + x0], v10 = map[(size_t)y1 * bw + x0];
        const float top = v00 + lx * (map[(size_t)y0 * bw + x1] - v00);
        const float bot = v10 + lx * (map[(size_t)y1 * bw + x1] - v10);
        const float up = top + ly * (bot - top);
        const size_t o = (size_t)y * W + x;
        if (image) {
            for (int c = 0; c < C; ++c) out[c * hw + o] = image[c * hw + o] + up;
        } else {
            out[o] = up;
        }
    }
}

// grid (ceil(bw / kBiasCells), bh): see the head of this file
__global__ __launch_bounds__(kBlock) void pixel_bias_bwd_kernel(int C, int H, int W, int n_cameras, int bh, int bw,
                                                                const int32_t *__restrict__ cam,
                                                                const float *__restrict__ g, float *__restrict__ grad_bias) {
    __shared__ float s_col[kBlock];
    const int tid = threadIdx.x;
    const int i = blockIdx.y;
    const int j0 = blockIdx.x * kBiasCells, j1 = min(j0 + kBiasCells, bw);
    const int j = j0 + tid;
    const bool cell = tid < kBiasCells && j < bw;
    const int ylo = bias_first(i - 1, bh, H), yhi = bias_first(i + 1, bh, H);
    const int xlo = bias_first(j0 - 1, bw, W), xhi = bias_first(j1, bw, W);      // the x range of cells j0 .. j1 - 1
    int cx0 = 0, cx1 = 0;
    if (cell) { cx0 = bias_first(j - 1, bw, W); cx1 = bias_first(j + 1, bw, W); }
    const size_t hw = (size_t)H * W;
    float acc = 0.f;
    for (int xb = xlo; xb < xhi; xb += kBlock) {
        const int x = xb + tid;
        float col = 0.f;
        if (x < xhi) {
            for (int y = ylo; y < yhi; ++y) {
                const float wy = bias_weight(y, i, bh, H);
                float s = 0.f;
                for (int c = 0; c < C; ++c) s += g[c * hw + (size_t)y * W + x];
                col = fmaf(wy, s, col);
            }
        }
        __syncthreads();                                     // the previous chunk's LDS reads are done
        s_col[tid] = col;
        __syncthreads();
        if (cell) {
            const int a = max(cx0, xb), e = min(cx1, min(xb + kBlock, xhi));
            for (int xx = a; xx < e; ++xx) acc = fmaf(bias_weight(xx, j, bw, W), s_col[xx - xb], acc);
        }
    }
    if (cell) {
        const int c = calib_cam(cam, 0, n_cameras);
        const size_t o = (size_t)i * bw + j, map = (size_t)bh * bw;
        for (int n = 0; n < n_cameras; ++n) grad_bias[n * map + o] = n == c ? acc : 0.f;
    }
}

}  // namespace d3ga

using namespace d3ga;

// segments and their length; < 0: the sizes are refused
static inline int calib_shape(int32_t k, int32_t n, int32_t planar, int32_t n_cameras, int32_t identity_idx, int *segs, int *L) {
    if (k < 1 || n < 0 || n_cameras < 1 || identity_idx >= n_cameras) return D3GA_E_SIZE;
    if (planar != 0 && planar != 1) return D3GA_E_CONFIG;
    if ((int64_t)k * 3 > kCalibRows) return D3GA_E_SIZE;
    if ((int64_t)n * 3 * k > INT32_MAX) return D3GA_E_SIZE;
    *segs = planar ? 3 * k : k;
    *L = planar ? n : 3 * n;
    return 0;
}

// workgroups per segment: one per tile, capped so that every workgroup of the launch has its row of partials
static inline int calib_grid(int L, int segs) {
    const int tiles = (L / 4 + kCalibTile - 1) / kCalibTile;
    const int cap = kCalibRows / segs;
    return tiles < 1 ? 1 : (tiles < cap ? tiles : cap);
}

extern "C" int d3ga_color_calib_fwd(int32_t k, int32_t n, int32_t planar, int32_t n_cameras, int32_t identity_idx,
                                    const float *rgb, const float *corrections, const int32_t *cam, float *out,
                                    d3ga_stream_t stream) {
    int segs, L;
    D3GA_TRY(calib_shape(k, n, planar, n_cameras, identity_idx, &segs, &L));
    if (!corrections || !cam) return D3GA_E_NULL;
    if (n == 0) return D3GA_OK;                              // (the element pointers of an empty tensor may be NULL)
    if (!rgb || !out) return D3GA_E_NULL;
    if (!aligned16(rgb) || !aligned16(out)) return D3GA_E_CONFIG;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(calib_grid(L, segs), segs);
    if (planar)
        hipLaunchKernelGGL((color_calib_kernel<false, true>), grid, dim3(kBlock), 0, s, L, n_cameras, identity_idx, rgb,
                           (const float *)nullptr, corrections, cam, out, (float *)nullptr);
    else
        hipLaunchKernelGGL((color_calib_kernel<false, false>), grid, dim3(kBlock), 0, s, L, n_cameras, identity_idx, rgb,
                           (const float *)nullptr, corrections, cam, out, (float *)nullptr);
    return check_launch(s, 0);
}

extern "C" int d3ga_color_calib_bwd(int32_t k, int32_t n, int32_t planar, int32_t n_cameras, int32_t identity_idx,
                                    float grad_scale, const float *rgb, const float *corrections, const int32_t *cam,
                                    const float *grad_out, float *grad_rgb, float *grad_corrections, float *partials,
                                    d3ga_stream_t stream) {
    int segs, L;
    D3GA_TRY(calib_shape(k, n, planar, n_cameras, identity_idx, &segs, &L));
    if (!corrections || !cam) return D3GA_E_NULL;
    if (n == 0 && !grad_corrections) return D3GA_OK;         // (the element pointers of an empty tensor may be NULL)
    if (n > 0 && !grad_out) return D3GA_E_NULL;
    if (!grad_rgb && !grad_corrections) return D3GA_E_NULL;
    if (grad_corrections && (!partials || (n > 0 && !rgb))) return D3GA_E_NULL;
    if (!aligned16(grad_out) || !aligned16(grad_rgb) || (grad_corrections && !aligned16(rgb))) return D3GA_E_CONFIG;
    hipStream_t s = (hipStream_t)stream;
    const int gx = calib_grid(L, segs);
    if (n > 0) {
        const dim3 grid(gx, segs);
        float *part = grad_corrections ? partials : (float *)nullptr;
        if (planar)
            hipLaunchKernelGGL((color_calib_kernel<true, true>), grid, dim3(kBlock), 0, s, L, n_cameras, identity_idx, grad_out,
                               rgb, corrections, cam, grad_rgb, part);
        else
            hipLaunchKernelGGL((color_calib_kernel<true, false>), grid, dim3(kBlock), 0, s, L, n_cameras, identity_idx, grad_out,
                               rgb, corrections, cam, grad_rgb, part);
    }
    if (grad_corrections)
        hipLaunchKernelGGL(color_calib_finish_kernel, dim3(1), dim3(kBlock), 0, s, k, n > 0 ? gx * (segs / k) : 0, n_cameras,
                           identity_idx, grad_scale, (const float *)partials, cam, grad_corrections);
    return check_launch(s, 0);
}

static inline int bias_shape(int32_t C, int32_t H, int32_t W, int32_t n_cameras, int32_t bh, int32_t bw) {
    if (C < 1 || H < 1 || W < 1 || n_cameras < 1 || bh < 1 || bw < 1) return D3GA_E_SIZE;
    if ((int64_t)C * H * W > INT32_MAX || (int64_t)n_cameras * bh * bw > INT32_MAX) return D3GA_E_SIZE;
    if ((int64_t)H * bh >= (1 << 30) || (int64_t)W * bw >= (1 << 30)) return D3GA_E_SIZE;      // the integer source coordinates
    return 0;
}

extern "C" int d3ga_pixel_bias_fwd(int32_t C, int32_t H, int32_t W, int32_t n_cameras, int32_t bh, int32_t bw,
                                   const float *bias, const int32_t *cam, const float *image, float *out,
                                   d3ga_stream_t stream) {
    D3GA_TRY(bias_shape(C, H, W, n_cameras, bh, bw));
    if (!bias || !cam || !out) return D3GA_E_NULL;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(pixel_bias_fwd_kernel, dim3((W + 63) / 64, (H + 15) / 16), dim3(kBlock), 0, s, C, H, W, n_cameras, bh, bw,
                       bias, cam, image, out);
    return check_launch(s, 0);
}

extern "C" int d3ga_pixel_bias_bwd(int32_t C, int32_t H, int32_t W, int32_t n_cameras, int32_t bh, int32_t bw,
                                   const int32_t *cam, const float *grad_out, float *grad_bias, d3ga_stream_t stream) {
    D3GA_TRY(bias_shape(C, H, W, n_cameras, bh, bw));
    if (!cam || !grad_out || !grad_bias) return D3GA_E_NULL;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(pixel_bias_bwd_kernel, dim3((bw + kBiasCells - 1) / kBiasCells, bh), dim3(kBlock), 0, s, C, H, W, n_cameras,
                       bh, bw, cam, grad_out, grad_bias);
    return check_launch(s, 0);
}
