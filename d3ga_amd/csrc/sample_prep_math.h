// sample_prep_math.h -- the rules of sample preparation (sample_prep.hip): what a loader worker does between the
// decoded uint8 arrays and the tensors of a sample (datasets/actorshq_dataset.py:244-276 with get_boundary_mask :201-217;
// datasets/goliath_dataset.py:454-481), restated per pixel.  Compiles for the host as it is: tests/hostcheck/sample_prep_host.cpp
// runs this very text on the CPU against tests/sample_prep_ref.py, and the kernels give its bytes.
//
// Everything is integer, or a multiple of 1/4 below 256 in float32: no rounding anywhere, so no compiler flag matters.
//
// ActorsHQ mode, per pixel, m = the matte's channel 0:
//   t         0 if m < 128, 1 if m > 128, 128 if m == 128 (the reference's two masked assignments leave that value alone)
//   er, di    the minimum and the maximum of t over the part of the 3 x 3 window that lies inside the image
//   boundary  uint8(di - er) == 1, or 5 < m < 250
//   fg        t == 1
//   label     0 without fg; else from (r, g, b) of seg -- all three taken as 127 when r + g + b == 0 -- in this order, the last
//             match winning: r == 255 -> 1, g == 255 -> 2, b == 255 -> 3, r == 127 -> 4
// Goliath mode: every output is the mean of a 2 x 2 block of uint8 values -- F.interpolate(scale_factor=0.5, mode="bilinear") of
// the float image, whose weights are 1/2 and 1/2 on rows 2 oy, 2 oy + 1 and columns 2 ox, 2 ox + 1; an odd last row or column is
// never read.
#pragma once
#include <stdint.h>

#include "../../include/d3ga.h"

#ifdef __HIPCC__
#define D3GA_FHD __host__ __device__ __forceinline__
#else
#define D3GA_FHD static inline
#endif

namespace d3ga {

// a uint8 source: pixel (b, y, x) starts at byte  p + b frame + y pitch + x step.  Nothing about p, pitch or frame is assumed to
// be a multiple of anything (an interleaved 747-wide row is 2241 bytes): every read is a byte read, and no byte outside a pixel
// that the rules name is ever touched.
struct SpSrc {
    const uint8_t *p;
    int64_t pitch, frame;
    int32_t step;
};

D3GA_FHD const uint8_t *sp_row(const SpSrc &s, int b, int y) { return s.p + (int64_t)b * s.frame + (int64_t)y * s.pitch; }

struct SpActors {
    int32_t B, H, W;
    SpSrc image, seg, mask;                                  // image, seg: step 3 (BGR); mask: step 1 or 3
    int32_t image_f32;                                       // image_out holds float32 instead of uint8
    void *image_out;                                         // (B,3,H,W) RGB
    int32_t *seg_part;                                       // (B,1,H,W)
    float *seg_fg, *boundary;                                // (B,1,H,W) 0 / 1
};

struct SpGoliath {
    int32_t B, H, W, oh, ow;
    SpSrc image, parts;                                      // planar, step 1
    int64_t image_plane;                                     // bytes between two channels of the image
    float *image_out;                                        // (B,3,oh,ow)
    float *seg_part, *seg_fg, *boundary;                     // (B,1,oh,ow)
};

D3GA_FHD int sp_imin(int a, int b) { return a < b ? a : b; }
D3GA_FHD int sp_imax(int a, int b) { return a > b ? a : b; }

D3GA_FHD int sp_thresh(int m) { return m < 128 ? 0 : (m > 128 ? 1 : 128); }

// with t in {0, 1, 128} the uint8 difference is 0, 1, 127 or 128
D3GA_FHD bool sp_boundary(int er, int di, int m) { return (uint8_t)(di - er) == 1 || (m > 5 && m < 250); }

D3GA_FHD int sp_label(int r, int g, int b) {
    if (r + g + b == 0) r = g = b = 127;
    int l = 0;
    if (r == 255) l = 1;
    if (g == 255) l = 2;
    if (b == 255) l = 3;
    if (r == 127) l = 4;
    return l;
}

struct SpPixel {
    uint8_t r, g, b, fg, boundary;
    int32_t label;
};

// colour, fg and label of pixel (y, x) once its matte value m is known; seg is read where there is foreground only
D3GA_FHD void sp_actors_colour(const uint8_t *image_row, const uint8_t *seg_row, int x, int m, SpPixel *o) {
    const uint8_t *ip = image_row + 3 * (int64_t)x;
    o->b = ip[0];
    o->g = ip[1];
    o->r = ip[2];
    o->fg = sp_thresh(m) == 1;
    o->label = 0;
    if (o->fg) {
        const uint8_t *sp = seg_row + 3 * (int64_t)x;
        o->label = sp_label(sp[2], sp[1], sp[0]);
    }
}

// one pixel: nine reads of the matte (those inside the image)
D3GA_FHD SpPixel sp_actors_pixel(const SpActors &a, int b, int y, int x) {
    int er = 255, di = 0, m = 0;
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = y + dy;
        if (yy < 0 || yy >= a.H) continue;
        const uint8_t *row = sp_row(a.mask, b, yy);
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = x + dx;
            if (xx < 0 || xx >= a.W) continue;
            const int v = row[(int64_t)xx * a.mask.step];
            const int t = sp_thresh(v);
            er = sp_imin(er, t);
            di = sp_imax(di, t);
            if (dy == 0 && dx == 0) m = v;
        }
    }
    SpPixel o;
    sp_actors_colour(sp_row(a.image, b, y), sp_row(a.seg, b, y), x, m, &o);
    o.boundary = sp_boundary(er, di, m);
    return o;
}

// four pixels x .. x + 3 of one row (x + 3 < W): eighteen reads of the matte instead of thirty-six, the same values
D3GA_FHD void sp_actors_quad(const SpActors &a, int b, int y, int x, SpPixel o[4]) {
    int er[4] = {255, 255, 255, 255}, di[4] = {0, 0, 0, 0}, m[4] = {0, 0, 0, 0};
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = y + dy;
        if (yy < 0 || yy >= a.H) continue;
        const uint8_t *row = sp_row(a.mask, b, yy);
        int lo[6], hi[6];                                    // t of columns x - 1 .. x + 4; outside the image neutral for min / max
        for (int j = 0; j < 6; ++j) {
            const int xx = x - 1 + j;
            lo[j] = 255;
            hi[j] = 0;
            if (xx >= 0 && xx < a.W) {
                const int v = row[(int64_t)xx * a.mask.step];
                lo[j] = hi[j] = sp_thresh(v);
                if (dy == 0 && j >= 1 && j <= 4) m[j - 1] = v;
            }
        }
        for (int k = 0; k < 4; ++k) {
            er[k] = sp_imin(er[k], sp_imin(lo[k], sp_imin(lo[k + 1], lo[k + 2])));
            di[k] = sp_imax(di[k], sp_imax(hi[k], sp_imax(hi[k + 1], hi[k + 2])));
        }
    }
    const uint8_t *image_row = sp_row(a.image, b, y), *seg_row = sp_row(a.seg, b, y);
    for (int k = 0; k < 4; ++k) {
        sp_actors_colour(image_row, seg_row, x + k, m[k], &o[k]);
        o[k].boundary = sp_boundary(er[k], di[k], m[k]);
    }
}

// the mean of four uint8 values: a multiple of 1/4 below 256, exact in float32 in any order of summation
D3GA_FHD float sp_mean4(int a, int b, int c, int d) { return (float)(a + b + c + d) * 0.25f; }

struct SpHalf {
    float rgb[3], part, fg;                                  // boundary = 1 - fg, exact as well
};

D3GA_FHD SpHalf sp_goliath_pixel(const SpGoliath &g, int b, int oy, int ox, bool with_image) {
    SpHalf o;
    const int64_t x = 2 * (int64_t)ox;
    for (int c = 0; c < 3; ++c) {
        o.rgb[c] = 0.f;
        if (!with_image) continue;
        const uint8_t *r0 = sp_row(g.image, b, 2 * oy) + c * g.image_plane + x, *r1 = r0 + g.image.pitch;
        o.rgb[c] = sp_mean4(r0[0], r0[1], r1[0], r1[1]);
    }
    const uint8_t *p0 = sp_row(g.parts, b, 2 * oy) + x, *p1 = p0 + g.parts.pitch;
    o.part = sp_mean4(p0[0], p0[1], p1[0], p1[1]);
    o.fg = sp_mean4(p0[0] != 0, p0[1] != 0, p1[0] != 0, p1[1] != 0);
    return o;
}

// ---- the argument rules of the two entry points (include/d3ga.h), shared with the host build; nothing is dereferenced ----------

// rows of `row` bytes, H of them per frame, B frames: the pitch holds a row, and with B > 1 the frame stride holds a frame
D3GA_FHD bool sp_src_fits(int64_t pitch, int64_t frame, int64_t row, int B, int H) {
    if (pitch < row) return false;
    return B == 1 || frame >= (int64_t)(H - 1) * pitch + row;
}

// *vec: the path of the launch.  1: four pixels per thread, 16-byte stores (4-byte ones for a uint8 image) -- W % 4 == 0 makes
// every row of every output plane start on the store's alignment; 0: a pixel per thread.
static inline int sp_plan_actorshq(int32_t B, int32_t H, int32_t W, int32_t Hs, int32_t Ws, const uint8_t *image, int64_t image_pitch,
                                   int64_t image_frame, const uint8_t *seg, int64_t seg_pitch, int64_t seg_frame, const uint8_t *mask,
                                   int64_t mask_pitch, int64_t mask_frame, int32_t mask_step, int32_t image_f32, void *image_out,
                                   int32_t *seg_part_out, float *seg_fg_out, float *boundary_out, SpActors *a, int32_t *vec) {
    if (B <= 0 || H <= 0 || W <= 0 || Hs <= 0 || Ws <= 0) return D3GA_E_SIZE;
    if (B > 65535 || (int64_t)H * W > INT32_MAX || (H + 3) / 4 > 65535) return D3GA_E_SIZE;      // the grid's z and y extents; 32-bit pixel indices
    if (Hs < H || Ws < W) return D3GA_E_SIZE;
    if (mask_step != 1 && mask_step != 3) return D3GA_E_CONFIG;
    if (image_f32 != 0 && image_f32 != 1) return D3GA_E_CONFIG;
    if (!sp_src_fits(image_pitch, image_frame, 3 * (int64_t)W, B, H) || !sp_src_fits(seg_pitch, seg_frame, 3 * (int64_t)Ws, B, H) ||
        !sp_src_fits(mask_pitch, mask_frame, (int64_t)(W - 1) * mask_step + 1, B, H))
        return D3GA_E_CONFIG;
    if (!image || !seg || !mask) return D3GA_E_NULL;
    if (!image_out && !seg_part_out && !seg_fg_out && !boundary_out) return D3GA_E_NULL;
    const uintptr_t words = (uintptr_t)seg_part_out | (uintptr_t)seg_fg_out | (uintptr_t)boundary_out | (image_f32 ? (uintptr_t)image_out : 0);
    if (words & 15) return D3GA_E_CONFIG;
    *a = {B, H, W, {image, image_pitch, image_frame, 3}, {seg, seg_pitch, seg_frame, 3}, {mask, mask_pitch, mask_frame, mask_step},
          image_f32, image_out, seg_part_out, seg_fg_out, boundary_out};
    *vec = W % 4 == 0 && ((uintptr_t)image_out & 3) == 0;
    return 0;
}

static inline int sp_plan_goliath(int32_t B, int32_t H, int32_t W, const uint8_t *image, int64_t image_pitch, int64_t image_plane,
                                  int64_t image_frame, const uint8_t *parts, int64_t parts_pitch, int64_t parts_frame, float *image_out,
                                  float *seg_part_out, float *seg_fg_out, float *boundary_out, SpGoliath *g, int32_t *vec) {
    if (B <= 0 || H < 2 || W < 2) return D3GA_E_SIZE;
    if (B > 65535 || (int64_t)H * W > INT32_MAX || (H / 2 + 3) / 4 > 65535) return D3GA_E_SIZE;
    if (image_plane < (int64_t)(H - 1) * image_pitch + W || !sp_src_fits(image_pitch, image_frame, W, B, H) ||
        (B > 1 && image_frame < 2 * image_plane + (int64_t)(H - 1) * image_pitch + W))
        return D3GA_E_CONFIG;
    if (!sp_src_fits(parts_pitch, parts_frame, W, B, H)) return D3GA_E_CONFIG;
    if (!image || !parts) return D3GA_E_NULL;
    if (!image_out && !seg_part_out && !seg_fg_out && !boundary_out) return D3GA_E_NULL;
    if (((uintptr_t)image_out | (uintptr_t)seg_part_out | (uintptr_t)seg_fg_out | (uintptr_t)boundary_out) & 15) return D3GA_E_CONFIG;
    *g = {B, H, W, H / 2, W / 2, {image, image_pitch, image_frame, 1}, {parts, parts_pitch, parts_frame, 1}, image_plane,
          image_out, seg_part_out, seg_fg_out, boundary_out};
    *vec = (W / 2) % 4 == 0;
    return 0;
}

}  // namespace d3ga
