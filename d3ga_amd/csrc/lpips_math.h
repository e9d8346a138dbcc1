// lpips_math.h -- the per-pixel arithmetic and the plans of the LPIPS (VGG) metric (lpips.hip), host-compilable: the text
// the kernels run is the text tests/hostcheck/lpips_check.cpp builds with g++ and holds against first-principles answers.
//
// The metric (R. Zhang et al., "The Unreasonable Effectiveness of Deep Features as a Perceptual Metric", 2018; the public
// `lpips` package, restated from recall -- DESIGN.md 4.4i, "parity unpinned"):
//     x' = ((normalize ? 2 x - 1 : x) - shift_c) / scale_c                                   the scaling layer
//     f_t = relu taps of VGG16 behind conv1_2, 2_2, 3_3, 4_3, 5_3                            13 convolutions, four 2x2 max pools
//     d_t(p) = sum_c lin_c ( a_c / (|a| + 1e-10) - b_c / (|b| + 1e-10) )^2                   a, b = f_t of the two images at pixel p
//     value = sum_t mean_p d_t(p)
// The difference is formed BEFORE the square: a == b gives exactly 0.  An all-zero feature vector has |a| = 0 and every
// a_c / 1e-10 = 0: that side contributes nothing, never a NaN.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LP_HD __host__ __device__ inline
#else
#define LP_HD inline
#endif

namespace d3ga {

constexpr int kLpConvs = 13;          // conv1_1 .. conv5_3 of VGG16
constexpr int kLpTaps = 5;
constexpr int kLpMinSide = 16;        // four floor pools: a side below 16 leaves nothing for the last tap
constexpr int kLpMaxC = 512;          // widest tap the distance kernel keeps in registers
constexpr int kLpPartials = 1024;     // most partial sums per image of the distance's spatial mean (D3GA_LPIPS_PARTIALS)
constexpr float kLpEps = 1e-10f;

// VGG16: a 2x2 max pool (floor) in FRONT of conv index 2, 4, 7, 10; a feature tap behind conv index 1, 3, 6, 9, 12.
LP_HD int lp_vgg16_width(int i) { return i < 2 ? 64 : (i < 4 ? 128 : (i < 7 ? 256 : 512)); }
LP_HD bool lp_pool_before(int i) { return i == 2 || i == 4 || i == 7 || i == 10; }
LP_HD bool lp_is_tap(int i) { return i == 1 || i == 3 || i == 6 || i == 9 || i == 12; }

// The scaling layer for channel c of an RGB image.
LP_HD float lp_input(float x, int c, int normalize) {
    const float shift = c == 0 ? -.030f : (c == 1 ? -.088f : -.188f);
    const float scale = c == 0 ? .458f : (c == 1 ? .448f : .450f);
    return ((normalize ? 2.f * x - 1.f : x) - shift) / scale;
}

// One channel's term of d(p), from the two norms |a| = sqrtf(sum a^2), |b|.
LP_HD float lp_term(float a, float b, float na, float nb, float lin) {
    const float d = a / (na + kLpEps) - b / (nb + kLpEps);
    return lin * (d * d);
}

// d(p) of one pixel with the channels in index order (the host's statement; the kernel sums the same terms in its lanes'
// order, lp_group_shift below).
LP_HD float lp_pixel_distance(int C, const float *a, const float *b, const float *lin) {
    float sa = 0.f, sb = 0.f, d = 0.f;
    for (int c = 0; c < C; ++c) { sa += a[c] * a[c]; sb += b[c] * b[c]; }
    const float na = sqrtf(sa), nb = sqrtf(sb);
    for (int c = 0; c < C; ++c) d += lp_term(a[c], b[c], na, nb, lin[c]);
    return d;
}

// The distance kernel gives a pixel a group of 2^shift lanes (vec: 4 consecutive channels per lane and pass, C % 4 == 0;
// else one), the smallest power of two that covers C in one pass, at most a wavefront: then kLpPassesVec / kLpPassesScalar
// passes cover kLpMaxC.
constexpr int kLpPassesVec = kLpMaxC / (64 * 4), kLpPassesScalar = kLpMaxC / 64;
LP_HD int lp_group_shift(int C, bool vec) {
    const int need = vec ? (C + 3) / 4 : C;
    int s = 0;
    while (s < 6 && (1 << s) < need) ++s;
    return s;
}
// workgroups per image: one per (256 >> shift) pixels, at most kLpPartials (each then strides over the image)
LP_HD int lp_tap_blocks(int64_t hw, int shift) {
    const int64_t ppb = 256 >> shift, n = (hw + ppb - 1) / ppb;
    return (int)(n < 1 ? 1 : (n > kLpPartials ? kLpPartials : n));
}

}  // namespace d3ga
