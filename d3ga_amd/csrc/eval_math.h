// eval_math.h -- the per-pixel arithmetic of the evaluation tail (eval.hip): the reference's test.py:140-141,151 (target
// composition), :186-187 (RGBA ground truth), recorder/heatmap.py:16-61 (the jet error heat map) and utils/image_utils.py:20-22
// (PSNR).  Compiles for the host as it is (tests/hostcheck/eval_host.cpp runs this very text on the CPU against
// tests/eval_ref.py).
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/d3ga.h"

#ifndef D3GA_FHD
#ifdef __HIPCC__
#define D3GA_FHD __host__ __device__ __forceinline__
#else
#define D3GA_FHD static inline
#endif
#endif

namespace d3ga {

// ---- how a frame is cut into workgroups ---------------------------------------------------------------------------------
// A workgroup of kEvalBlock threads walks `passes` passes of kEvalPass pixels (four pixels per thread and pass) and leaves
// ONE squared-error partial per channel.  passes = 4 up to 8.4 M pixels (a 4K frame), more behind that, so that a channel
// never has more than kEvalMaxPartials partials.
constexpr int kEvalBlock = 256;
constexpr int kEvalPass = 4 * kEvalBlock;
constexpr int kEvalMinPasses = 4;
constexpr int kEvalMaxPartials = D3GA_EVAL_MAX_PARTIALS;
constexpr int64_t kEvalMaxPixels = (int64_t)1 << 26;          // H W beyond this is refused (D3GA_E_SIZE)

D3GA_FHD int eval_passes(int64_t hw) {
    const int64_t p = (hw + (int64_t)kEvalPass * kEvalMaxPartials - 1) / ((int64_t)kEvalPass * kEvalMaxPartials);
    return p < kEvalMinPasses ? kEvalMinPasses : (int)p;
}
// partials per (frame, channel) = workgroups per frame
D3GA_FHD int eval_partials(int64_t hw) {
    const int64_t chunk = (int64_t)kEvalPass * eval_passes(hw);
    return (int)((hw + chunk - 1) / chunk);
}

// ---- the jet table ----------------------------------------------------------------------------------------------------
// dist_to_rgb (recorder/heatmap.py:26-34) maps an error through matplotlib's "jet" at N = 256 and truncates colour * 255 to
// uint8.  The table is restated here from jet's piecewise-linear segments the way matplotlib builds its lookup table
// (colors._create_lookup_table: x = 255 data_x, xind = 255 (i / 255), searchsorted from the left, linear in between, the
// first and last entries taken from the ends, clipped to [0, 1]), all in double and at compile time, so the host and the
// device hold the same 257 x 3 bytes: row 256 is the "bad" colour a NaN error takes (transparent black).
struct JetKnot {
    double x, y;
};
struct JetTable {
    uint8_t v[257][3];
};

constexpr double jet_lut_entry(const JetKnot *d, int n, int i) {
    double v = 0.0;
    if (i == 0) {
        v = d[0].y;
    } else if (i == 255) {
        v = d[n - 1].y;
    } else {
        const double xi = 255.0 * ((double)i * (1.0 / 255.0));          // 255 * numpy.linspace(0, 1, 256)[i]
        int k = 0;
        while (k < n - 1 && d[k].x * 255.0 < xi) ++k;                   // searchsorted(x, xi, "left")
        const double x0 = d[k - 1].x * 255.0, x1 = d[k].x * 255.0;
        const double t = (xi - x0) / (x1 - x0);
        v = t * (d[k].y - d[k - 1].y) + d[k - 1].y;
    }
    return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
}

constexpr JetTable make_jet_table() {
    constexpr JetKnot r[] = {{0, 0}, {.35, 0}, {.66, 1}, {.89, 1}, {1, .5}};
    constexpr JetKnot g[] = {{0, 0}, {.125, 0}, {.375, 1}, {.64, 1}, {.91, 0}, {1, 0}};
    constexpr JetKnot b[] = {{0, .5}, {.11, 1}, {.34, 1}, {.65, 0}, {1, 0}};
    JetTable t = {};
    for (int i = 0; i < 256; ++i) {
        t.v[i][0] = (uint8_t)(jet_lut_entry(r, 5, i) * 255.0);
        t.v[i][1] = (uint8_t)(jet_lut_entry(g, 6, i) * 255.0);
        t.v[i][2] = (uint8_t)(jet_lut_entry(b, 5, i) * 255.0);
    }
    t.v[256][0] = t.v[256][1] = t.v[256][2] = 0;
    return t;
}

constexpr int kJetBad = 256;
// the colour the heat map stores: uint8 / 255 in float32 (heatmap.py:47)
D3GA_FHD float jet_colour(uint8_t v) { return (float)v / 255.0f; }

// ---- per pixel --------------------------------------------------------------------------------------------------------
// Every operation is rounded to float32 on its own, in the reference's order (separate ATen / numpy kernels there).
struct EvalPixel {
    float target[3];     // image a + (1 - a) bg, or the image itself when it is already composed
    float gt[4];         // image a, a                                  (composition only)
    float sq[3];         // (target - pred)^2 per channel
    int bin;             // row of the jet table
};

// heatmap.py:26-34: clip(0, 1, e) there is min(1, e); bin = int(e 256), 256 -> 255; NaN -> the bad colour
D3GA_FHD int eval_error_bin(float e) {
    if (e != e) return kJetBad;
    const int i = (int)(fminf(e, 1.0f) * 256.0f);
    return i < 255 ? i : 255;
}

// heatmap.py:45: e = ||target - pred||_2 over the channels, from the three squares
D3GA_FHD int eval_heat_bin(float s0, float s1, float s2) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    return eval_error_bin(sqrtf((s0 + s1) + s2));
}

// one channel of a pixel: fills target[c], gt[c] and sq[c]
D3GA_FHD void eval_channel(bool composed, float bg, float a, float pred, float image, int c, EvalPixel *o) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const float fg = composed ? image : image * a;
    const float t = composed ? image : fg + (1.0f - a) * bg;  // test.py:151
    const float d = t - pred;
    o->gt[c] = fg;
    o->target[c] = t;
    o->sq[c] = d * d;
}

// boundary: float(boundary_fg) of the pixel; alpha0: channel 0 of alpha (test.py:140-141).  (Written out per channel: a loop
// over c would index the arrays at run time, which costs the kernel a stack frame.)
D3GA_FHD void eval_pixel(bool composed, float bg, float p0, float p1, float p2, float i0, float i1, float i2, float alpha0,
                         float boundary, EvalPixel *o) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const float a = composed ? 1.0f : alpha0 * (1.0f - boundary);
    eval_channel(composed, bg, a, p0, i0, 0, o);
    eval_channel(composed, bg, a, p1, i1, 1, o);
    eval_channel(composed, bg, a, p2, i2, 2, o);
    o->gt[3] = a;
    o->bin = eval_heat_bin(o->sq[0], o->sq[1], o->sq[2]);
}

// ---- SSIM, forward only, one 16 x 16 tile of one channel -------------------------------------------------------------------
// utils/loss_utils.py:46-86: the 11 x 11 window gaussian(11, 1.5) (x) gaussian(11, 1.5), zero padding of 5, C1 = 0.01^2,
// C2 = 0.03^2.  The window is separable: the tile's 26 x 26 inputs of both images go to `x` and `y`, the five maps (x, y, x^2,
// y^2, xy) are convolved horizontally into `h` (5 planes of 26 rows x 16 columns) and vertically per output pixel.  Returns the
// sum of ssim_map over the in-image pixels THIS thread owns (pixel i of the tile belongs to thread i % nthr); sync() is the
// workgroup barrier (nothing on the host, where tid = 0 and nthr = 1).  The evaluation sums these per tile and stores the
// partial plainly: d3ga_ssim_fwd (loss.hip) adds its workgroups' sums with float atomics, so its last bits follow arrival order.
constexpr int kEvalSsimTile = 16, kEvalSsimHalo = 5, kEvalSsimIn = kEvalSsimTile + 2 * kEvalSsimHalo;
constexpr int kEvalSsimInputs = kEvalSsimIn * kEvalSsimIn, kEvalSsimRows = kEvalSsimIn * kEvalSsimTile;

D3GA_FHD float eval_ssim_weight(int k) {      // gaussian(11, 1.5) normalised in float32, the numbers loss.hip uses
    const float w[11] = {1.028380124e-03f, 7.598758209e-03f, 3.600077331e-02f, 1.093606874e-01f, 2.130055279e-01f, 2.660117149e-01f,
                         2.130055279e-01f, 1.093606874e-01f, 3.600077331e-02f, 7.598758209e-03f, 1.028380124e-03f};
    return w[k];
}

D3GA_FHD int64_t eval_ssim_tiles(int H, int W) {
    return (int64_t)((H + kEvalSsimTile - 1) / kEvalSsimTile) * ((W + kEvalSsimTile - 1) / kEvalSsimTile);
}

template <class Sync>
D3GA_FHD float eval_ssim_tile(float *x, float *y, float *h, const float *img1, const float *img2, int H, int W, int ty0, int tx0, int tid,
                              int nthr, Sync sync) {
    for (int i = tid; i < kEvalSsimInputs; i += nthr) {
        const int ry = i / kEvalSsimIn, rx = i - ry * kEvalSsimIn;
        const int gy = ty0 - kEvalSsimHalo + ry, gx = tx0 - kEvalSsimHalo + rx;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        x[i] = in ? img1[(size_t)gy * W + gx] : 0.f;
        y[i] = in ? img2[(size_t)gy * W + gx] : 0.f;
    }
    sync();
    for (int i = tid; i < kEvalSsimRows; i += nthr) {
        const int ry = i / kEvalSsimTile, ox = i - ry * kEvalSsimTile;
        float m1 = 0.f, m2 = 0.f, q1 = 0.f, q2 = 0.f, q12 = 0.f;
        for (int k = 0; k < 11; ++k) {
            const float w = eval_ssim_weight(k), a = x[ry * kEvalSsimIn + ox + k], b = y[ry * kEvalSsimIn + ox + k];
            m1 += w * a; m2 += w * b; q1 += w * (a * a); q2 += w * (b * b); q12 += w * (a * b);
        }
        h[i] = m1; h[kEvalSsimRows + i] = m2; h[2 * kEvalSsimRows + i] = q1; h[3 * kEvalSsimRows + i] = q2; h[4 * kEvalSsimRows + i] = q12;
    }
    sync();
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    float sum = 0.f;
    for (int i = tid; i < kEvalSsimTile * kEvalSsimTile; i += nthr) {
        const int oy = i / kEvalSsimTile, ox = i - oy * kEvalSsimTile;
        if (ty0 + oy >= H || tx0 + ox >= W) continue;
        float m1 = 0.f, m2 = 0.f, q1 = 0.f, q2 = 0.f, q12 = 0.f;
        for (int k = 0; k < 11; ++k) {
            const float w = eval_ssim_weight(k);
            const int r = (oy + k) * kEvalSsimTile + ox;
            m1 += w * h[r]; m2 += w * h[kEvalSsimRows + r]; q1 += w * h[2 * kEvalSsimRows + r]; q2 += w * h[3 * kEvalSsimRows + r];
            q12 += w * h[4 * kEvalSsimRows + r];
        }
        const float m11 = m1 * m1, m22 = m2 * m2, m12 = m1 * m2;
        const float s1 = q1 - m11, s2 = q2 - m22, s12 = q12 - m12;
        sum += ((2.f * m12 + C1) * (2.f * s12 + C2)) / ((m11 + m22 + C1) * (s1 + s2 + C2));
    }
    return sum;
}

// 20 log10(1 / sqrt(mse)) (utils/image_utils.py:22) = -10 log10(mse), taken in double: mse = 0 gives +inf, as in torch
D3GA_FHD double eval_psnr_db(float mse) { return -10.0 * log10((double)mse); }

}  // namespace d3ga
