// frame_prep_math.h -- the per-pixel arithmetic and the window-count stages of frame preparation (frame_prep.hip), the
// image path of the reference's Batcher.process (lib/batch.py:150-163, 180, 205-208, 236).  Compiles for the host as it is
// (tests/hostcheck/frame_prep_host.cpp runs this very text on the CPU, one "thread", against tests/frame_ref.py).
//
// Masks are 0 / 1 bytes, four pixels to a 32-bit word (byte j of a word = pixel x + j; little-endian hosts only), so a
// window count is a sum of whole words: no byte ever exceeds 49 and nothing carries into its neighbour.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/d3ga.h"

#ifdef __HIPCC__
#define D3GA_FHD __host__ __device__ __forceinline__
#else
#define D3GA_FHD static inline
#endif

namespace d3ga {

constexpr int kFrameTileW = 64;                              // output tile of one workgroup
constexpr int kFrameTileH = 32;
constexpr int kFrameMaxHalo = 12;                            // 3 (median) + 5 (erode_mask) + 4 (close_holes)
constexpr int kFrameCols = kFrameTileW + 2 * kFrameMaxHalo;  // the planes always carry the widest halo in x: a constant row length
constexpr int kFrameWpr = kFrameCols / 4;                    // words per plane row
constexpr int kFramePlaneWords = (kFrameTileH + 2 * kFrameMaxHalo) * kFrameWpr;
constexpr int kFrameMaxStages = 5;

// one window-count stage: out = (number of ones in the (2r + 1)^2 window >= thresh); a pixel outside the image is written as
// pad_out, the value the NEXT stage wants to read there
//   median 7x7    r 3, thresh 25  (zero padding: the input outside the image is 0)
//   dilation      thresh 1        (in-image window: outside reads as 0)
//   erosion       thresh (2r+1)^2 (in-image window: outside reads as 1)
struct FrameStage {
    int r, thresh, pad_out;
};

// The stages in the reference's order (median, erode_mask, close_holes) occupy five fixed slots: 0 the median, 1 and 2 the 7x7
// dilation and 5x5 erosion of erode_mask (utils/image_utils.py:49-58), 3 and 4 the 5x5 pair of close_holes (:61-70).  Returns
// whether slot k is switched on by `flags`.  A dilation (slots 1, 3) is always followed by its erosion, hence its pad_out.
D3GA_FHD bool frame_stage_at(int flags, int k, FrameStage *st) {
    const int r = (k == 0 || k == 1) ? 3 : 2;
    *st = {r, k == 0 ? 25 : ((k & 1) ? 1 : (2 * r + 1) * (2 * r + 1)), (k & 1) ? 1 : 0};
    return k == 0 || (k <= 2 ? (flags & D3GA_FRAME_ERODE_MASK) != 0 : (flags & D3GA_FRAME_CLOSE_HOLES) != 0);
}

// rows of halo the stages of `flags` consume: the sum of their radii
D3GA_FHD int frame_halo(int flags) {
    return 3 + ((flags & D3GA_FRAME_ERODE_MASK) ? 5 : 0) + ((flags & D3GA_FRAME_CLOSE_HOLES) ? 4 : 0);
}

// .int() of a float label: truncation toward zero
D3GA_FHD int frame_label(float v) { return (int)v; }

// lib/batch.py:154
D3GA_FHD uint8_t frame_fg(int s, float seg_fg) { return (uint8_t)((s > 0) | (seg_fg > 0.f)); }

// row of the colour table a label selects: 0 background, s for 0 < s < n_labels, n_labels ("other") for every other label
D3GA_FHD int frame_sil_index(int s, int n_labels) { return s == 0 ? 0 : (s > 0 && s < n_labels ? s : n_labels); }

D3GA_FHD float frame_sil(int idx, int c, const float *label_rgb, int n_labels, const float *other_rgb, float bg) {
    return idx == 0 ? bg : (idx < n_labels ? label_rgb[3 * idx + c] : other_rgb[c]);
}

// calibrate_color (lib/batch.py:78-88) of one value of channel c: v / 255, and with use_gamma_space linear2color_corr
// (utils/image_utils.py:92-113).  Every operation is rounded to float32 on its own, in the reference's order.
D3GA_FHD float frame_orig(float v, int c, bool gamma) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const float x = v / 255.0f;
    if (!gamma) return x;
    const float black = (float)(3.0 / 255.0);
    const float k = (float)((1.0 / (1.0 - 3.0 / 255.0)) * 0.95);
    const float scale = c == 0 ? 1.4f : (c == 1 ? 1.1f : 1.6f);
    const float lin = (x * scale) / 1.1f;
    const float t = fminf(fmaxf(lin - black, 0.f), 2.f);
    const float g = sqrtf(k * t) - (float)(15.0 / 255.0);
    return fminf(fmaxf(g, 0.f), 2.f);
}

// byte j = 1 iff pixel (y, x + j) lies inside the image
D3GA_FHD uint32_t frame_inside(int y, int x, int H, int W) {
    if (y < 0 || y >= H) return 0u;
    uint32_t m = 0u;
    for (int j = 0; j < 4; ++j)
        if (x + j >= 0 && x + j < W) m |= 1u << (8 * j);
    return m;
}

// the counts of the 2r + 1 pixels around each of the four pixels of word c (l, rt: the words to its left and right), r <= 3
D3GA_FHD uint32_t frame_row_count(uint32_t l, uint32_t c, uint32_t rt, int r) {
    uint32_t s = c;
    for (int d = 1; d <= r; ++d) {
        s += (c >> (8 * d)) | (rt << (32 - 8 * d));          // pixel x + d
        s += (c << (8 * d)) | (l >> (32 - 8 * d));           // pixel x - d
    }
    return s;
}

// the rule: byte = (count >= thresh), counts and thresh in [0, 49] (count + 128 - thresh stays inside the byte)
D3GA_FHD uint32_t frame_rule(uint32_t counts, int thresh) {
    return ((counts + 0x80808080u - 0x01010101u * (uint32_t)thresh) >> 7) & 0x01010101u;
}

// One stage over a plane of `rows` rows of kFrameWpr words whose first pixel is (y0, x0) of the image: row counts into
// `cnt`, then column counts and the rule back into `plane`.  What lies outside the PLANE counts as 0, so after the stage the
// outermost st.r rows and columns are not valid any more: the caller's halo is the sum of the radii.  `tid` of `nthr`
// threads share the work; sync() is the workgroup barrier (nothing on the host, where tid = 0 and nthr = 1).
template <class Sync>
D3GA_FHD void frame_stage(uint32_t *plane, uint32_t *cnt, int rows, int y0, int x0, int H, int W, FrameStage st, int tid, int nthr,
                          Sync sync) {
    const int n = rows * kFrameWpr;
    for (int i = tid; i < n; i += nthr) {
        const int w = i % kFrameWpr;
        cnt[i] = frame_row_count(w > 0 ? plane[i - 1] : 0u, plane[i], w + 1 < kFrameWpr ? plane[i + 1] : 0u, st.r);
    }
    sync();
    for (int i = tid; i < n; i += nthr) {
        const int y = i / kFrameWpr, w = i - y * kFrameWpr;
        uint32_t s = 0u;
        for (int dy = -st.r; dy <= st.r; ++dy)
            if (y + dy >= 0 && y + dy < rows) s += cnt[i + dy * kFrameWpr];
        const uint32_t m = frame_inside(y0 + y, x0 + 4 * w, H, W);
        plane[i] = (frame_rule(s, st.thresh) & m) | (st.pad_out ? (0x01010101u & ~m) : 0u);
    }
    sync();
}

// The masks of the tile whose first pixel is (ty0, tx0) of image b.  Loads fg (lib/batch.py:154; 0 outside the image: kornia's
// median pads with zeros) with a halo of *halo rows and kFrameMaxHalo columns into `plane`, keeps the tile's own fg bytes and
// colour-table rows in fg_tile / labels (kFrameTileW * kFrameTileH each), and runs the stages when with_alpha is set.
// Afterwards alpha of tile pixel (ty, tx) is byte (ty + *halo) * kFrameCols + tx + kFrameMaxHalo of the plane.
template <class Sync>
D3GA_FHD void frame_tile_masks(uint32_t *plane, uint32_t *cnt, int32_t *labels, uint8_t *fg_tile, int flags, bool with_alpha, int b,
                               int H, int W, int ty0, int tx0, const void *seg_part, const float *seg_fg, int n_labels, int tid,
                               int nthr, Sync sync, int *halo) {
    const int h = with_alpha ? frame_halo(flags) : 0;
    const int rows = kFrameTileH + 2 * h;
    uint8_t *pb = reinterpret_cast<uint8_t *>(plane);
    for (int i = tid; i < rows * kFrameCols; i += nthr) {
        const int ry = i / kFrameCols, rx = i - ry * kFrameCols;
        const int y = ty0 - h + ry, x = tx0 - kFrameMaxHalo + rx;
        uint8_t f = 0;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const size_t o = ((size_t)b * H + y) * W + x;
            const int s = (flags & D3GA_FRAME_SEG_F32) ? frame_label(static_cast<const float *>(seg_part)[o])
                                                       : static_cast<const int32_t *>(seg_part)[o];
            f = frame_fg(s, seg_fg ? seg_fg[o] : 0.f);
            const int ty = ry - h, tx = rx - kFrameMaxHalo;
            if (ty >= 0 && ty < kFrameTileH && tx >= 0 && tx < kFrameTileW) {
                labels[ty * kFrameTileW + tx] = frame_sil_index(s, n_labels);
                fg_tile[ty * kFrameTileW + tx] = f;
            }
        }
        pb[i] = f;
    }
    sync();
    for (int k = 0; with_alpha && k < kFrameMaxStages; ++k) {
        FrameStage st;
        if (frame_stage_at(flags, k, &st)) frame_stage(plane, cnt, rows, ty0 - h, tx0 - kFrameMaxHalo, H, W, st, tid, nthr, sync);
    }
    *halo = h;
}

}  // namespace d3ga
