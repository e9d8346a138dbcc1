// perceptual.hip -- the VGG19 perceptual loss of the reference (utils/loss_utils.py:109-160 VGGLoss; train.py:212-214):
// 13 3x3 convolutions conv1_1 .. conv5_1 with ReLU, four 2x2 max pools, a 2x2 box downsize in front and an L1 mean per
// feature tap.  The weights are frozen, so only the input gradient exists, and the input gradient of a 3x3, stride-1,
// pad-1 convolution is the same convolution over dY (.) [Y > 0] with flipped, transposed weights: ONE kernel template does
// both directions, as linear_kernel of mlp.hip does for the field networks.
//
// conv3x3_kernel: implicit GEMM on v_mfma_f32_32x32x16_bf16, M = pixels, N = Cout, K = 9 Cin in the unit order of
// perceptual_math.h (a unit = 8 consecutive channels of one tap of one pixel = 32 contiguous bytes of the channels-last
// activation).  A wavefront owns 32 pixels x NB column blocks of 32; a workgroup is four such wavefronts on consecutive
// pixel rows of the GEMM (they share the weight slots through the cache, nothing through LDS, so there is no barrier and a
// wavefront past the last pixel simply leaves).  Lane l feeds the MFMA with the 8 k of pixel l & 31, k-half l >> 5: it
// loads its own 32 bytes (two 16-byte loads when Cin % 8 == 0), zeroes what the mask says, splits every f32 exactly into
// three bf16 pieces and multiplies the six products with i + j <= 2 against the three weight planes -- f32-equivalent
// arithmetic (mlp.hip's header has the error analysis and the 2.7x over the f32-input MFMA).
// PREDICATION: every tap outside the image, every pixel past H W, every channel past Cin and every unit past 9 Cu is
// decided BEFORE the load and never read; column blocks past Cout are clamped to the last real block (whose slots exist)
// and never stored.  The next k-step's loads are issued before the current one is multiplied.
//
// Layout: activations are channels-last (H, W, C) f32.  The image enters as (3, H, W): box_down2 does the transpose.
//
// BATCH (d3ga_vgg_conv3x3_n, d3ga_vgg_maxpool2_fwd_n): N images (N, H, W, C) ride in the GEMM's M dimension, row
// p = (n H + y) W + x, so a wavefront's 32 pixels may span two images and the N images share every weight load.  A lane takes
// its pixel apart into (n, y, x) once; the zero padding is decided from (y, x) alone, so a tap never crosses a seam, and a row
// of the MFMA depends on nothing but its own pixel: image n of a batch is bit for bit the single-image call on that image.
// The single-image entry points are the N = 1 case of the same kernels.
#include "d3ga_internal.h"
#include "perceptual_math.h"

namespace d3ga {

using pc_f32x16 = __attribute__((ext_vector_type(16))) float;
typedef __bf16 pc_bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 pc_bf16x8 __attribute__((ext_vector_type(8)));
typedef float pc_f32x2 __attribute__((ext_vector_type(2)));
constexpr int kConvThreads = 256;    // 4 wavefronts x 32 pixels
constexpr int kConvRows = 128;
constexpr int kConvFlush = 8;       // k-steps (128 k) per chunk of the two-level sum; a power of two

__device__ __forceinline__ uint32_t pc_pack(float a, float b) {
    pc_f32x2 v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, pc_bf16x2));     // round to nearest even
}
// (x, y) = p0 + p1 + p2 exactly, each piece a bf16 pair: the remainders of a round-to-nearest are representable
__device__ __forceinline__ void pc_split2(float x, float y, uint32_t &p0, uint32_t &p1, uint32_t &p2) {
    p0 = pc_pack(x, y);
    const float r0 = x - __builtin_bit_cast(float, p0 << 16), r1 = y - __builtin_bit_cast(float, p0 & 0xffff0000u);
    p1 = pc_pack(r0, r1);
    p2 = pc_pack(r0 - __builtin_bit_cast(float, p1 << 16), r1 - __builtin_bit_cast(float, p1 & 0xffff0000u));
}
__device__ __forceinline__ void pc_split8(const float (&v)[8], uint4 &q0, uint4 &q1, uint4 &q2) {
    pc_split2(v[0], v[1], q0.x, q1.x, q2.x);
    pc_split2(v[2], v[3], q0.y, q1.y, q2.y);
    pc_split2(v[4], v[5], q0.z, q1.z, q2.z);
    pc_split2(v[6], v[7], q0.w, q1.w, q2.w);
}

// One thread per 16-byte slot of a plane (perceptual_math.h: pc_panel_source).
__global__ __launch_bounds__(kBlock) void pc_pack_kernel(int w_cout, int w_cin, int transposed, int64_t plane_slots,
                                                         const float *__restrict__ Wt, uint4 *__restrict__ panel) {
    const int64_t slot = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (slot >= plane_slots) return;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int64_t src = pc_panel_source(w_cout, w_cin, transposed, slot, j);
        v[j] = src >= 0 ? Wt[src] : 0.f;
    }
    uint4 q0, q1, q2;
    pc_split8(v, q0, q1, q2);
    panel[slot] = q0;
    panel[plane_slots + slot] = q1;
    panel[2 * plane_slots + slot] = q2;
}

template <int NB>
struct ConvRaw {
    float4 a0, a1, m0, m1;
    uint4 w[NB][3];
};

template <int NB, bool VEC, bool MASK>
__global__ __launch_bounds__(kConvThreads) void conv3x3_kernel(int M, int H, int W, int Cin, int Cout, const float *__restrict__ X,
                                                               const float *__restrict__ Ym, const uint4 *__restrict__ panel,
                                                               const float *__restrict__ bias, int relu, int accumulate,
                                                               float *__restrict__ Y) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l32 = lane & 31;
    const int row0 = ((int)blockIdx.x * 4 + wave) * 32;
    if (row0 >= M) return;                                            // wave-uniform; the kernel has no barrier
    const int cu = pc_units_per_tap(Cin), KK = pc_ksteps(Cin), nbt = pc_nblocks(Cout);
    const int64_t plane = (int64_t)KK * 2 * nbt * 32;
    const int p = row0 + l32;
    const bool prow = p < M;
    const int HW = H * W;                                             // M = N HW rows, image after image
    const int pn = prow ? p / HW : 0, pq = p - pn * HW;
    const int py = prow ? pq / W : 0, px = prow ? pq - py * W : 0;
    const size_t img0 = (size_t)pn * (size_t)HW;                      // first row of this pixel's image
    int nbg[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) nbg[nb] = min((int)blockIdx.y * NB + nb, nbt - 1);
    pc_f32x16 acc[NB], tot[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nb][r] = tot[nb][r] = 0.f;

    // this lane's unit u = 2 kk + half as (tap, c8), advanced by two units per k-step
    int tap = 0, c8 = half;
    while (c8 >= cu) { c8 -= cu; ++tap; }
    auto load = [&](int kk, ConvRaw<NB> &r) __attribute__((always_inline)) {
        const int ky = tap / 3, kx = tap - 3 * ky;
        const int yy = py + ky - 1, xx = px + kx - 1;
        const bool ok = prow && tap < 9 && yy >= 0 && yy < H && xx >= 0 && xx < W;
        r.a0 = r.a1 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (MASK) r.m0 = r.m1 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok) {
            const size_t o = (img0 + (size_t)yy * (size_t)W + (size_t)xx) * (size_t)Cin + (size_t)c8 * 8;
            if constexpr (VEC) {                                       // Cin % 8 == 0: 32-byte aligned, all 8 channels exist
                r.a0 = *reinterpret_cast<const float4 *>(X + o);
                r.a1 = *reinterpret_cast<const float4 *>(X + o + 4);
                if constexpr (MASK) {
                    r.m0 = *reinterpret_cast<const float4 *>(Ym + o);
                    r.m1 = *reinterpret_cast<const float4 *>(Ym + o + 4);
                }
            } else {
                const int left = Cin - c8 * 8;                         // >= 1: c8 < cu
                float e[8], m[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    e[j] = j < left ? X[o + j] : 0.f;
                    m[j] = (MASK && j < left) ? Ym[o + j] : 0.f;
                }
                r.a0 = make_float4(e[0], e[1], e[2], e[3]);
                r.a1 = make_float4(e[4], e[5], e[6], e[7]);
                if constexpr (MASK) {
                    r.m0 = make_float4(m[0], m[1], m[2], m[3]);
                    r.m1 = make_float4(m[4], m[5], m[6], m[7]);
                }
            }
        }
        const uint4 *wp = panel + ((size_t)(2 * kk + half) * (size_t)nbt) * 32 + l32;      // 2 kk + half < 2 KK: the slot exists
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) r.w[nb][pl] = wp[pl * plane + nbg[nb] * 32];
        c8 += 2;
        while (c8 >= cu) { c8 -= cu; ++tap; }
    };

    ConvRaw<NB> cur, nxt;
    load(0, cur);
    for (int kk = 0; kk < KK; ++kk) {
        if (kk + 1 < KK) load(kk + 1, nxt);
        float v[8] = {cur.a0.x, cur.a0.y, cur.a0.z, cur.a0.w, cur.a1.x, cur.a1.y, cur.a1.z, cur.a1.w};
        if constexpr (MASK) {
            const float m[8] = {cur.m0.x, cur.m0.y, cur.m0.z, cur.m0.w, cur.m1.x, cur.m1.y, cur.m1.z, cur.m1.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = m[j] > 0.f ? v[j] : 0.f;
        }
        uint4 q[3];
        pc_split8(v, q[0], q[1], q[2]);
        pc_bf16x8 a[3];
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) a[pl] = __builtin_bit_cast(pc_bf16x8, q[pl]);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            pc_bf16x8 w[3];
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) w[pl] = __builtin_bit_cast(pc_bf16x8, cur.w[nb][pl]);
            // smallest products first
            acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], w[0], acc[nb], 0, 0, 0);
            acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], w[1], acc[nb], 0, 0, 0);
            acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], w[2], acc[nb], 0, 0, 0);
            acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], w[0], acc[nb], 0, 0, 0);
            acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], w[1], acc[nb], 0, 0, 0);
            acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], w[0], acc[nb], 0, 0, 0);
        }
        // Two-level sum: the MFMA accumulator runs over kConvFlush k-steps only, then joins `tot` through a rounded VALU add.
        // One accumulator over all of K = 9 Cin (864 dependent MFMAs at Cin = 256) left 5x the error of a blocked float32
        // sum on the CPU; the chunks keep the chain short and the partial sums small.
        if ((kk & (kConvFlush - 1)) == kConvFlush - 1) {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int r = 0; r < 16; ++r) { tot[nb][r] += acc[nb][r]; acc[nb][r] = 0.f; }
        }
        if (kk + 1 < KK) cur = nxt;
    }

    // C/D layout of the 32x32 shapes: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5): every store
    // instruction covers two 128-byte segments of two pixels
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int n = ((int)blockIdx.y * NB + nb) * 32 + l32;
        if (n >= Cout) continue;
        const float b = bias ? bias[n] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = row0 + 4 * half + (r & 3) + 8 * (r >> 2);
            if (row >= M) continue;
            const size_t o = (size_t)row * (size_t)Cout + (size_t)n;
            float y = (tot[nb][r] + acc[nb][r]) + b;
            if (relu) y = y > 0.f ? y : 0.f;
            if (accumulate) y += Y[o];
            Y[o] = y;
        }
    }
}

// 2x2 max pool, stride 2, floor; channels-last, N images back to back.  One thread per output element.
__global__ __launch_bounds__(kBlock) void pc_pool_fwd_kernel(int N, int H, int W, int C, const float *__restrict__ x, float *__restrict__ y) {
    const int Ho = H / 2, Wo = W / 2;
    const int64_t n = (int64_t)N * Ho * Wo * C;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int c = (int)(i % C);
        const int64_t q = i / C;
        const int ox = (int)(q % Wo);
        const int64_t r = q / Wo;
        const int oy = (int)(r % Ho), im = (int)(r / Ho);
        const float *s = x + (((int64_t)im * H + 2 * oy) * W + 2 * ox) * C + c;
        const float a = s[0], b = s[C], d = s[(int64_t)W * C], e = s[(int64_t)W * C + C];
        y[i] = fmaxf(fmaxf(a, b), fmaxf(d, e));
    }
}
// One thread per INPUT element: the gradient of its window if it is the window's first maximum in row-major order
// (torch's rule), zero otherwise and in the odd last row / column that the floor drops.
__global__ __launch_bounds__(kBlock) void pc_pool_bwd_kernel(int H, int W, int C, const float *__restrict__ x,
                                                             const float *__restrict__ gy, float *__restrict__ gx) {
    const int Ho = H / 2, Wo = W / 2;
    const int64_t n = (int64_t)H * W * C;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int c = (int)(i % C);
        const int64_t q = i / C;
        const int ix = (int)(q % W), iy = (int)(q / W);
        const int ox = ix >> 1, oy = iy >> 1;
        float g = 0.f;
        if (ox < Wo && oy < Ho) {
            const float *s = x + ((int64_t)(2 * oy) * W + 2 * ox) * C + c;
            const float v[4] = {s[0], s[C], s[(int64_t)W * C], s[(int64_t)W * C + C]};
            int best = 0;
#pragma unroll
            for (int k = 1; k < 4; ++k)
                if (v[k] > v[best]) best = k;
            if (best == 2 * (iy & 1) + (ix & 1)) g = gy[((int64_t)oy * Wo + ox) * C + c];
        }
        gx[i] = g;
    }
}

// (C, H, W) image -> channels-last (Ho, Wo, C): the 2x2 box mean of x[:2 Ho, :2 Wo] (down), or the transpose alone.
__global__ __launch_bounds__(kBlock) void pc_down_fwd_kernel(int C, int H, int W, int down, const float *__restrict__ img,
                                                             float *__restrict__ out) {
    const int Ho = down ? H / 2 : H, Wo = down ? W / 2 : W;
    const int64_t n = (int64_t)Ho * Wo * C;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int c = (int)(i % C);
        const int64_t q = i / C;
        const int ox = (int)(q % Wo), oy = (int)(q / Wo);
        const float *s = img + (int64_t)c * H * W;
        if (down) {
            const float *t = s + (int64_t)(2 * oy) * W + 2 * ox;
            out[i] = 0.25f * ((t[0] + t[1]) + (t[W] + t[W + 1]));
        } else {
            out[i] = s[(int64_t)oy * W + ox];
        }
    }
}
// One thread per element of the (C, H, W) gradient; exact zeros in the dropped row and column.
__global__ __launch_bounds__(kBlock) void pc_down_bwd_kernel(int C, int H, int W, int down, const float *__restrict__ g,
                                                             float *__restrict__ g_img) {
    const int Ho = down ? H / 2 : H, Wo = down ? W / 2 : W;
    const int64_t n = (int64_t)C * H * W;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int ix = (int)(i % W);
        const int64_t q = i / W;
        const int iy = (int)(q % H), c = (int)(q / H);
        const int ox = down ? ix >> 1 : ix, oy = down ? iy >> 1 : iy;
        float v = 0.f;
        if (ox < Wo && oy < Ho) {
            v = g[((int64_t)oy * Wo + ox) * C + c];
            if (down) v *= 0.25f;
        }
        g_img[i] = v;
    }
}

template <int NB>
static void launch_conv(bool vec, bool mask, dim3 grid, hipStream_t s, int M, int H, int W, int cin, int cout, const float *x,
                        const float *mask_y, const uint4 *panel, const float *bias, int relu, int accumulate, float *y) {
#define D3GA_PC_LAUNCH(V, K) \
    hipLaunchKernelGGL((conv3x3_kernel<NB, V, K>), grid, dim3(kConvThreads), 0, s, M, H, W, cin, cout, x, mask_y, panel, bias, relu, accumulate, y)
    if (vec && mask) D3GA_PC_LAUNCH(true, true);
    else if (vec) D3GA_PC_LAUNCH(true, false);
    else if (mask) D3GA_PC_LAUNCH(false, true);
    else D3GA_PC_LAUNCH(false, false);
#undef D3GA_PC_LAUNCH
}

// sizes of N channels-last activations: positive, and every element index of the batch fits an int32
static inline bool pc_sizes_ok(int64_t H, int64_t W, int64_t C, int64_t N = 1) {
    return N > 0 && H > 0 && W > 0 && C > 0 && H * W <= INT32_MAX && N * H * W <= INT32_MAX && N * H * W * C <= INT32_MAX;
}

}  // namespace d3ga

using namespace d3ga;

extern "C" int64_t d3ga_vgg_panel_bytes(int32_t cin, int32_t cout) {
    if (cin <= 0 || cout <= 0 || cin > (1 << 20) || cout > (1 << 20)) return D3GA_E_SIZE;
    return pc_panel_bytes(cin, cout);
}

extern "C" int d3ga_vgg_pack_weights(int32_t w_cout, int32_t w_cin, const float *weight, int32_t transposed, void *panel,
                                     d3ga_stream_t stream) {
    if (w_cout <= 0 || w_cin <= 0 || w_cout > (1 << 20) || w_cin > (1 << 20)) return D3GA_E_SIZE;
    if (!weight || !panel) return D3GA_E_NULL;
    if (transposed != 0 && transposed != 1) return D3GA_E_CONFIG;
    if ((uintptr_t)panel & 15) return D3GA_E_CONFIG;
    const int64_t slots = transposed ? pc_plane_slots(w_cout, w_cin) : pc_plane_slots(w_cin, w_cout);
    if (slots > INT32_MAX) return D3GA_E_SIZE;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(pc_pack_kernel, dim3((unsigned)((slots + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, w_cout, w_cin,
                       transposed, slots, weight, reinterpret_cast<uint4 *>(panel));
    return check_launch(s, 0);
}

extern "C" int d3ga_vgg_conv3x3_n(int32_t N, int32_t H, int32_t W, int32_t cin, int32_t cout, const float *x, const float *mask_y,
                                  const void *panel, const float *bias, int32_t relu, int32_t accumulate, float *y,
                                  d3ga_stream_t stream) {
    if (!pc_sizes_ok(H, W, cin, N) || !pc_sizes_ok(H, W, cout, N)) return D3GA_E_SIZE;
    if (pc_plane_slots(cin, cout) > INT32_MAX) return D3GA_E_SIZE;
    if (!x || !panel || !y) return D3GA_E_NULL;
    if ((relu & ~1) || (accumulate & ~1)) return D3GA_E_CONFIG;
    if (((uintptr_t)x | (uintptr_t)mask_y | (uintptr_t)panel) & 15) return D3GA_E_CONFIG;       // 16-byte loads
    if (((uintptr_t)y | (uintptr_t)bias) & 3) return D3GA_E_CONFIG;
    if (y == x || y == mask_y) return D3GA_E_CONFIG;                   // a pixel's neighbours read what another wavefront writes
    hipStream_t s = (hipStream_t)stream;
    const int nbt = pc_nblocks(cout);
    const int NB = nbt >= 3 ? 4 : nbt;
    const int M = N * H * W;
    const dim3 grid((unsigned)(((int64_t)M + kConvRows - 1) / kConvRows), (unsigned)((nbt + NB - 1) / NB));
    const bool vec = (cin & 7) == 0, mask = mask_y != nullptr;
    const uint4 *pn = reinterpret_cast<const uint4 *>(panel);
    if (NB == 1) launch_conv<1>(vec, mask, grid, s, M, H, W, cin, cout, x, mask_y, pn, bias, relu, accumulate, y);
    else if (NB == 2) launch_conv<2>(vec, mask, grid, s, M, H, W, cin, cout, x, mask_y, pn, bias, relu, accumulate, y);
    else launch_conv<4>(vec, mask, grid, s, M, H, W, cin, cout, x, mask_y, pn, bias, relu, accumulate, y);
    return check_launch(s, 0);
}

extern "C" int d3ga_vgg_conv3x3(int32_t H, int32_t W, int32_t cin, int32_t cout, const float *x, const float *mask_y,
                                const void *panel, const float *bias, int32_t relu, int32_t accumulate, float *y,
                                d3ga_stream_t stream) {
    return d3ga_vgg_conv3x3_n(1, H, W, cin, cout, x, mask_y, panel, bias, relu, accumulate, y, stream);
}

extern "C" int d3ga_vgg_maxpool2_fwd_n(int32_t N, int32_t H, int32_t W, int32_t C, const float *x, float *y, d3ga_stream_t stream) {
    if (!pc_sizes_ok(H, W, C, N) || H < 2 || W < 2) return D3GA_E_SIZE;
    if (!x || !y) return D3GA_E_NULL;
    if (x == y) return D3GA_E_CONFIG;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(pc_pool_fwd_kernel, dim3(grid_1d((int64_t)N * (H / 2) * (W / 2) * C)), dim3(kBlock), 0, s, N, H, W, C, x, y);
    return check_launch(s, 0);
}

extern "C" int d3ga_vgg_maxpool2_fwd(int32_t H, int32_t W, int32_t C, const float *x, float *y, d3ga_stream_t stream) {
    if (!pc_sizes_ok(H, W, C) || H < 2 || W < 2) return D3GA_E_SIZE;
    if (!x || !y) return D3GA_E_NULL;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(pc_pool_fwd_kernel, dim3(grid_1d((int64_t)(H / 2) * (W / 2) * C)), dim3(kBlock), 0, s, 1, H, W, C, x, y);
    return check_launch(s, 0);
}

extern "C" int d3ga_vgg_maxpool2_bwd(int32_t H, int32_t W, int32_t C, const float *x, const float *gy, float *gx,
                                     d3ga_stream_t stream) {
    if (!pc_sizes_ok(H, W, C) || H < 2 || W < 2) return D3GA_E_SIZE;
    if (!x || !gy || !gx) return D3GA_E_NULL;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(pc_pool_bwd_kernel, dim3(grid_1d((int64_t)H * W * C)), dim3(kBlock), 0, s, H, W, C, x, gy, gx);
    return check_launch(s, 0);
}

extern "C" int d3ga_vgg_box_down2_fwd(int32_t C, int32_t H, int32_t W, int32_t down, const float *img, float *out,
                                      d3ga_stream_t stream) {
    if (!pc_sizes_ok(H, W, C) || (down && (H < 2 || W < 2))) return D3GA_E_SIZE;
    if (!img || !out) return D3GA_E_NULL;
    if (down & ~1) return D3GA_E_CONFIG;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = down ? (int64_t)(H / 2) * (W / 2) * C : (int64_t)H * W * C;
    hipLaunchKernelGGL(pc_down_fwd_kernel, dim3(grid_1d(n)), dim3(kBlock), 0, s, C, H, W, down, img, out);
    return check_launch(s, 0);
}

extern "C" int d3ga_vgg_box_down2_bwd(int32_t C, int32_t H, int32_t W, int32_t down, const float *g, float *g_img,
                                      d3ga_stream_t stream) {
    if (!pc_sizes_ok(H, W, C) || (down && (H < 2 || W < 2))) return D3GA_E_SIZE;
    if (!g || !g_img) return D3GA_E_NULL;
    if (down & ~1) return D3GA_E_CONFIG;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(pc_down_bwd_kernel, dim3(grid_1d((int64_t)H * W * C)), dim3(kBlock), 0, s, C, H, W, down, g, g_img);
    return check_launch(s, 0);
}

extern "C" int d3ga_vgg_scratch_bytes(int32_t H, int32_t W, int32_t down, int32_t n_layers, const int32_t *widths, int64_t *out) {
    if (!out) return D3GA_E_NULL;
    if (H <= 0 || W <= 0 || (int64_t)H * W > INT32_MAX / 3) return D3GA_E_SIZE;
    if (n_layers < 1 || n_layers > kVggTaps || (down & ~1)) return D3GA_E_CONFIG;
    const int nc = pc_convs_for_layers(n_layers);
    int64_t h = H, w = W;
    if (down) { h /= 2; w /= 2; }
    if (h < 1 || w < 1) return D3GA_E_SIZE;
    int64_t saved = align256(4 * h * w * 3), biggest = h * w * 3;
    int c_prev = 3;
    for (int i = 0; i < nc; ++i) {
        const int c = widths ? widths[i] : pc_vgg19_width(i);
        if (c <= 0) return D3GA_E_SIZE;
        if (pc_pool_before(i)) {
            h /= 2; w /= 2;
            if (h < 1 || w < 1) return D3GA_E_SIZE;
            saved += align256(4 * h * w * c_prev);
        }
        if (h * w * c > INT32_MAX) return D3GA_E_SIZE;
        saved += align256(4 * h * w * c) * (pc_is_tap(i) ? 2 : 1);      // a tap keeps its L1 gradient next to the activation
        if (h * w * c > biggest) biggest = h * w * c;
        c_prev = c;
    }
    out[0] = saved;                                                                  // source activations and tap gradients, kept for the backward
    out[1] = 2 * align256(4 * biggest) + align256(4 * D3GA_LOSS_PARTIALS) + 256;    // target ping-pong | L1 partials | tap means
    out[2] = 2 * align256(4 * biggest);                                              // gradient ping-pong of the backward
    return D3GA_OK;
}
