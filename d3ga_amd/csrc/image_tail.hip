// image_tail.hip -- the image tail of the Goliath configuration, between render() and the losses.
//   blur_mix_*      models/learnable_blur.py:34-44 (called at models/trainer.py:124-126): a per-camera softmax mix of the
//                   rendered image, its 3x3 and its 7x7 Gaussian blur (torchvision's gaussian_blur: reflect padding).
//   compose_target  train.py:182-188: target image and silhouette target from image, alpha, boundary mask and background.
//
// The blur.  B_k = separable Gaussian of k taps, g_k[i] ~ exp(-(x_i / sigma_k)^2 / 2), x_i = i - (k - 1) / 2, normalised,
// sigma_k = 0.15 k + 0.35, over the image extended by k / 2 pixels of REFLECT padding (index -1 -> 1, n -> n - 2).  Taps,
// sigma rule and padding are recalled from torchvision (not part of the reference tree): DESIGN.md sec. 2.
//
// One kernel serves both directions.  Per axis the blur is A = K R (R: reflect extension, K: the taps), and for a symmetric
// K and n >= k / 2 + 1 its adjoint is  A^T = S A E  with E = diag(2, 1, ..., 1, 2) and S = diag(1/2, 1, ..., 1, 1/2): the
// reflect extension is self-adjoint under the inner product that counts the two edge samples half (the whole-sample
// symmetric extension of the DCT-I).  Element by element, A[m,i] = k[m-i] + [i>=1] k[m+i] + [i<=n-2] k[2(n-1)-m-i] and
// A^T[m,i] is the same with the brackets on m; the two differ only where m or i is an edge sample, by exactly the factors
// of S and E (the third term vanishes against an edge because 2(n-1) - (n-2) = n > k / 2).  In two dimensions S, A and E
// are tensor products, so the backward is the forward's tile code on the upstream gradient staged with the edge rows and
// columns doubled, with the results of the edge rows and columns halved -- the gradient that falls on the padded ring is
// folded back onto rows / columns 1..k/2 (and their counterparts at the far edge), and row 0 receives none of it.
//
// A workgroup (256 threads) owns a 64 x 32 output tile of one channel: the tile plus a 3-pixel halo goes to LDS once,
// the horizontal pass forms both blur widths from it (four outputs per thread, 16-byte LDS reads and writes), the
// vertical pass forms eight outputs per thread (one column, 32 LDS reads per eight pixels) and mixes.
// HBM traffic per pixel and channel: forward 4 B read + 4 B written, backward 8 B read + 4 B written.
#include "d3ga_internal.h"
#include "wave_prims.h"

namespace d3ga {

constexpr int kBlurTW = 64, kBlurTH = 32, kBlurHalo = 3;
constexpr int kBlurInH = kBlurTH + 2 * kBlurHalo;          // 38 staged rows
constexpr int kBlurInLd = 72;                              // floats per staged row: 70 columns, padded (16-byte aligned rows, 12 floats from any quad)
static_assert(kBlurTW + 2 * kBlurHalo <= kBlurInLd && kBlurTW + 8 <= kBlurInLd, "staged row too short");
constexpr int kBlurRows = kBlurTH / 4;                     // output rows per thread of the vertical pass (four wavefronts)
constexpr int kBlurGridCap = D3GA_BLUR_PARTIALS / 3;       // workgroups of a launch: three partial sums each

// gaussian(3, 0.8) and gaussian(7, 1.4), centre first (float64 values rounded once)
constexpr float kG3_0 = 0.52201146875401892f, kG3_1 = 0.23899426562299048f;
constexpr float kG7_0 = 0.28802604575225105f, kG7_1 = 0.22317336074208335f, kG7_2 = 0.10381835124997371f,
                kG7_3 = 0.028995265131817438f;

// reflect without repeating the edge sample; positions further out than the padding (tiles that hang over the image: they
// only feed pixels that are never written) are clamped into the image
__device__ __forceinline__ int reflect_idx(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * n - 2 - i : i;
    return min(max(i, 0), n - 1);
}

// the camera's row of weights_raw -> softmax; an index outside [0, n_cameras) is clamped (the Python layer validates
// host-side integers; a device-side index is the caller's)
__device__ __forceinline__ void blur_weights(const float *__restrict__ weights_raw, const int32_t *__restrict__ cam_idx,
                                             int n_cameras, float (&w)[3]) {
    const int cam = min(max(cam_idx[0], 0), n_cameras - 1);
    const float r0 = weights_raw[3 * cam], r1 = weights_raw[3 * cam + 1], r2 = weights_raw[3 * cam + 2];
    const float m = fmaxf(r0, fmaxf(r1, r2));
    const float e0 = expf(r0 - m), e1 = expf(r1 - m), e2 = expf(r2 - m);
    const float inv = 1.0f / (e0 + e1 + e2);
    w[0] = e0 * inv; w[1] = e1 * inv; w[2] = e2 * inv;
}

// BWD = false: src = img, dst = out = w0 img + w1 B3 img + w2 B7 img.
// BWD = true:  src = dL/dout, dst = dL/dimg = w0 g + w1 B3^T g + w2 B7^T g (NULL: skipped); with img != NULL the three sums
//              <g, img>, <B3^T g, img>, <B7^T g, img> of this workgroup's tiles go to partials[3 * blockIdx.x + 0..2].
template <bool BWD>
__global__ __launch_bounds__(256) void blur_mix_kernel(int C, int H, int W, int tiles_x, int tiles_y, int n_cameras,
                                                       const float *__restrict__ src, const float *__restrict__ img,
                                                       const float *__restrict__ weights_raw,
                                                       const int32_t *__restrict__ cam_idx, float *__restrict__ dst,
                                                       float *__restrict__ partials) {
    __shared__ __attribute__((aligned(16))) float s_in[kBlurInH][kBlurInLd];
    __shared__ __attribute__((aligned(16))) float s_h3[kBlurInH][kBlurTW], s_h7[kBlurInH][kBlurTW];
    __shared__ float s_part[3][4];
    const int tid = threadIdx.x;
    float w[3];
    blur_weights(weights_raw, cam_idx, n_cameras, w);
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f;
    const int per_plane = tiles_x * tiles_y, ntiles = C * per_plane;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int c = t / per_plane, r = t - c * per_plane;
        const int ty = r / tiles_x, tx = r - ty * tiles_x;
        const size_t plane = (size_t)c * H * W;
        const int x0 = tx * kBlurTW, y0 = ty * kBlurTH;
        __syncthreads();                                   // the previous tile's LDS reads are done
        for (int idx = tid; idx < kBlurInH * kBlurInLd; idx += 256) {
            const int rr = idx / kBlurInLd, cc = idx - rr * kBlurInLd;
            const int gy = reflect_idx(y0 + rr - kBlurHalo, H), gx = reflect_idx(x0 + cc - kBlurHalo, W);
            float v = src[plane + (size_t)gy * W + gx];    // (the two pad columns hold in-image values nobody reads)
            if (BWD) {
                if (gy == 0 || gy == H - 1) v *= 2.f;      // E: the edge samples count twice
                if (gx == 0 || gx == W - 1) v *= 2.f;
            }
            s_in[rr][cc] = v;
        }
        __syncthreads();
        // horizontal pass: thread = (staged row, four adjacent output columns)
        for (int it = tid; it < kBlurInH * (kBlurTW / 4); it += 256) {
            const int rr = it >> 4, c0 = 4 * (it & 15);
            float v[12];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float4 q = *reinterpret_cast<const float4 *>(&s_in[rr][c0 + 4 * j]);
                v[4 * j] = q.x; v[4 * j + 1] = q.y; v[4 * j + 2] = q.z; v[4 * j + 3] = q.w;
            }
            float h3[4], h7[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {                  // output column c0 + j: staged columns c0 + j .. c0 + j + 6, centre + 3
                h3[j] = kG3_0 * v[j + 3] + kG3_1 * (v[j + 2] + v[j + 4]);
                h7[j] = kG7_0 * v[j + 3] + kG7_1 * (v[j + 2] + v[j + 4]) + kG7_2 * (v[j + 1] + v[j + 5]) + kG7_3 * (v[j] + v[j + 6]);
            }
            *reinterpret_cast<float4 *>(&s_h3[rr][c0]) = make_float4(h3[0], h3[1], h3[2], h3[3]);
            *reinterpret_cast<float4 *>(&s_h7[rr][c0]) = make_float4(h7[0], h7[1], h7[2], h7[3]);
        }
        __syncthreads();
        // vertical pass: thread = one column, kBlurRows consecutive output rows (a wavefront reads 64 consecutive floats)
        const int px = tid & 63, py0 = kBlurRows * (tid >> 6);
        const int gx = x0 + px;
        float a7[kBlurRows + 6], a3[kBlurRows + 2];
#pragma unroll
        for (int k = 0; k < kBlurRows + 6; ++k) a7[k] = s_h7[py0 + k][px];
#pragma unroll
        for (int k = 0; k < kBlurRows + 2; ++k) a3[k] = s_h3[py0 + 2 + k][px];
        const float sx = (BWD && (gx == 0 || gx == W - 1)) ? 0.5f : 1.f;          // S: ... and receive half
#pragma unroll
        for (int i = 0; i < kBlurRows; ++i) {
            const int gy = y0 + py0 + i;
            float t0 = s_in[py0 + i + kBlurHalo][px + kBlurHalo];
            float t1 = kG3_0 * a3[i + 1] + kG3_1 * (a3[i] + a3[i + 2]);
            float t2 = kG7_0 * a7[i + 3] + kG7_1 * (a7[i + 2] + a7[i + 4]) + kG7_2 * (a7[i + 1] + a7[i + 5]) + kG7_3 * (a7[i] + a7[i + 6]);
            if (gy < H && gx < W) {
                const size_t o = plane + (size_t)gy * W + gx;
                if (BWD) {
                    const float s = (gy == 0 || gy == H - 1) ? 0.5f * sx : sx;
                    t0 *= s; t1 *= s; t2 *= s;
                    if (img) {
                        const float x = img[o];
                        acc0 = fmaf(t0, x, acc0); acc1 = fmaf(t1, x, acc1); acc2 = fmaf(t2, x, acc2);
                    }
                }
                if (dst) dst[o] = w[0] * t0 + w[1] * t1 + w[2] * t2;
            }
        }
    }
    if (BWD && img) {                                      // one partial per workgroup and sum: plain stores, fixed order
        acc0 = wave_sum(acc0); acc1 = wave_sum(acc1); acc2 = wave_sum(acc2);
        if ((tid & 63) == 0) { s_part[0][tid >> 6] = acc0; s_part[1][tid >> 6] = acc1; s_part[2][tid >> 6] = acc2; }
        __syncthreads();
        if (tid < 3) partials[3 * blockIdx.x + tid] = (s_part[tid][0] + s_part[tid][1]) + (s_part[tid][2] + s_part[tid][3]);
    }
}

// finishing stage: ONE workgroup adds the partials in index order, applies the softmax Jacobian and writes the whole
// (n_cameras, 3) gradient -- the camera's row, exact zeros everywhere else (no memset by the caller)
__global__ __launch_bounds__(kBlock) void blur_finish_kernel(int np, const float *__restrict__ partials, int n_cameras,
                                                             const float *__restrict__ weights_raw,
                                                             const int32_t *__restrict__ cam_idx,
                                                             float *__restrict__ grad_weights_raw) {
    __shared__ float s_part[3][kBlock / 64];
    __shared__ float s_grad[3];
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int i = threadIdx.x; i < np; i += kBlock) { a0 += partials[3 * i]; a1 += partials[3 * i + 1]; a2 += partials[3 * i + 2]; }
    a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2);
    if ((threadIdx.x & 63) == 0) { s_part[0][threadIdx.x >> 6] = a0; s_part[1][threadIdx.x >> 6] = a1; s_part[2][threadIdx.x >> 6] = a2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float s[3], w[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float t = 0.f;
#pragma unroll
            for (int k = 0; k < kBlock / 64; ++k) t += s_part[j][k];
            s[j] = t;
        }
        blur_weights(weights_raw, cam_idx, n_cameras, w);
        const float mean = w[0] * s[0] + w[1] * s[1] + w[2] * s[2];
#pragma unroll
        for (int j = 0; j < 3; ++j) s_grad[j] = w[j] * (s[j] - mean);
    }
    __syncthreads();
    const int cam = min(max(cam_idx[0], 0), n_cameras - 1);
    for (int i = threadIdx.x; i < 3 * n_cameras; i += kBlock) grad_weights_raw[i] = (i / 3 == cam) ? s_grad[i - 3 * cam] : 0.f;
}

// train.py:182-188:  m = 1 - boundary_fg;  gt = (image alpha + (1 - alpha) bg_c) m + (1 - m) bg_c;  sil = silhouette alpha m
template <typename MaskT>
__global__ __launch_bounds__(kBlock) void compose_target_kernel(int C, int64_t hw, const float *__restrict__ image,
                                                                const float *__restrict__ alpha,
                                                                const float *__restrict__ silhouette,
                                                                const MaskT *__restrict__ boundary_fg,
                                                                const float *__restrict__ bg, float *__restrict__ gt_image,
                                                                float *__restrict__ gt_silhouette) {
#pragma clang fp contract(off)                             // every product rounded, as the reference's separate ATen kernels do
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < hw; i += stride) {
        const float a = alpha[i], m = 1.f - (float)boundary_fg[i];
        for (int c = 0; c < C; ++c) {
            const float b = bg[c];
            const size_t o = (size_t)c * hw + i;
            const float g = image[o] * a + (1.f - a) * b;
            gt_image[o] = g * m + (1.f - m) * b;
            gt_silhouette[o] = silhouette[o] * a * m;
        }
    }
}

}  // namespace d3ga

using namespace d3ga;

static inline int blur_tiles(int C, int H, int W, int *tx, int *ty) {
    *tx = (W + kBlurTW - 1) / kBlurTW;
    *ty = (H + kBlurTH - 1) / kBlurTH;
    return C * *tx * *ty;
}

extern "C" int d3ga_blur_mix_fwd(int32_t C, int32_t H, int32_t W, int32_t n_cameras, const float *img,
                                 const float *weights_raw, const int32_t *cam_idx, float *out, d3ga_stream_t stream) {
    if (C <= 0 || H < 4 || W < 4 || n_cameras <= 0) return D3GA_E_SIZE;
    if ((int64_t)C * H * W > INT32_MAX) return D3GA_E_SIZE;
    if (!img || !weights_raw || !cam_idx || !out) return D3GA_E_NULL;
    hipStream_t s = (hipStream_t)stream;
    int tx, ty;
    const int ntiles = blur_tiles(C, H, W, &tx, &ty);
    hipLaunchKernelGGL(blur_mix_kernel<false>, dim3(ntiles < kBlurGridCap ? ntiles : kBlurGridCap), dim3(256), 0, s, C, H, W, tx, ty,
                       n_cameras, img, (const float *)nullptr, weights_raw, cam_idx, out, (float *)nullptr);
    return check_launch(s, 0);
}

extern "C" int d3ga_blur_mix_bwd(int32_t C, int32_t H, int32_t W, int32_t n_cameras, const float *img,
                                 const float *weights_raw, const int32_t *cam_idx, const float *grad_out, float *grad_img,
                                 float *grad_weights_raw, float *partials, d3ga_stream_t stream) {
    if (C <= 0 || H < 4 || W < 4 || n_cameras <= 0) return D3GA_E_SIZE;
    if ((int64_t)C * H * W > INT32_MAX) return D3GA_E_SIZE;
    if (!weights_raw || !cam_idx || !grad_out) return D3GA_E_NULL;
    if (!grad_img && !grad_weights_raw) return D3GA_E_NULL;
    if (grad_weights_raw && (!img || !partials)) return D3GA_E_NULL;
    hipStream_t s = (hipStream_t)stream;
    int tx, ty;
    const int ntiles = blur_tiles(C, H, W, &tx, &ty);
    const int grid = ntiles < kBlurGridCap ? ntiles : kBlurGridCap;
    hipLaunchKernelGGL(blur_mix_kernel<true>, dim3(grid), dim3(256), 0, s, C, H, W, tx, ty, n_cameras, grad_out,
                       grad_weights_raw ? img : (const float *)nullptr, weights_raw, cam_idx, grad_img, partials);
    if (grad_weights_raw)
        hipLaunchKernelGGL(blur_finish_kernel, dim3(1), dim3(kBlock), 0, s, grid, (const float *)partials, n_cameras, weights_raw,
                           cam_idx, grad_weights_raw);
    return check_launch(s, 0);
}

extern "C" int d3ga_compose_target(int32_t C, int32_t H, int32_t W, const float *image, const float *alpha,
                                   const float *silhouette, const void *boundary_fg, int32_t boundary_is_float,
                                   const float *bg, float *gt_image, float *gt_silhouette, d3ga_stream_t stream) {
    if (C <= 0 || H <= 0 || W <= 0) return D3GA_E_SIZE;
    if (!image || !alpha || !silhouette || !boundary_fg || !bg || !gt_image || !gt_silhouette) return D3GA_E_NULL;
    hipStream_t s = (hipStream_t)stream;
    const int64_t hw = (int64_t)H * W;
    const int64_t blocks = (hw + kBlock - 1) / kBlock;
    const dim3 grid((unsigned)(blocks > 8192 ? 8192 : blocks));
    if (boundary_is_float)
        hipLaunchKernelGGL(compose_target_kernel<float>, grid, dim3(kBlock), 0, s, C, hw, image, alpha, silhouette,
                           (const float *)boundary_fg, bg, gt_image, gt_silhouette);
    else
        hipLaunchKernelGGL(compose_target_kernel<uint8_t>, grid, dim3(kBlock), 0, s, C, hw, image, alpha, silhouette,
                           (const uint8_t *)boundary_fg, bg, gt_image, gt_silhouette);
    return check_launch(s, 0);
}
