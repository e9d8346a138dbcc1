// frame_grid_math.h -- the arithmetic of the recorder's frame grid (frame_grid.hip): the label layout of write_text
// (utils/text_helpers.py:27-50) in the project's own units, glyph coverage, the blend, the two uint8 quantisers and the "{:.3f}"
// formatter.  Semantics: DESIGN.md 4.4o (specification of record).  Compiles for the host as it is
// (tests/hostcheck/gridcheck.cpp runs this very text on the CPU); frame_grid.hip is compiled with -ffp-contract=off, so the
// device evaluates every float32 expression here as g++ does.
//
//   unit        u = min(w / 150, 17.7): 25 cells of 6 u fit in a panel w pixels wide (fg_unit); the bound is the reference's
//               largest font scale 5.9 in units of u (its baseline sits 30 scale below the top, ours 10 u: u = 3 scale)
//   baseline    int(10 u) below the panel's top, or h - int(5 u) with `bottom`; the glyph rows 0..6 end on it (cap height 7 u)
//   line        the label is ONE bitmap of 6 n columns by 7 rows: column G belongs to character G / 6, the sixth column of a
//               cell is empty.  Texel (G, r) has its centre at (G + 0.5, r + 0.5) units from (X, baseline - 7 u)
//   coverage    the bilinear sample of that bitmap at the pixel's centre, texels outside it 0 (fg_sample); bold: the larger of
//               the sample and the sample half a unit to the left (the glyph united with itself half a unit to the right)
//   blend       alpha > 0 ? (1 - alpha) x + alpha colour : x  -- a pixel the text does not reach keeps its bits
//   quantisers  fg_quant_save_image: uint8(clamp(fl(fl(255 x) + 0.5), 0, 255)); fg_quant_clip: uint8(clamp(fl(255 x), 0, 255));
//               NaN -> 0 in both (torch and numpy leave that conversion undefined)
//   number      fg_format: q = rint(|x| 1000) in float64 (the product is exact for a float32 x; rint is half-to-even), clamped
//               to 999999999; sign, integer digits, '.', three decimals; nan, inf, -inf as Python prints them
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/d3ga.h"
#include "frame_grid_font.h"

#ifndef D3GA_FHD
#ifdef __HIPCC__
#define D3GA_FHD __host__ __device__ __forceinline__
#else
#define D3GA_FHD static inline
#endif
#endif
// what reads the font table: device-only under hipcc (the table is a __device__ constant there)
#ifdef __HIPCC__
#define D3GA_FG_DEV __device__ __forceinline__
#else
#define D3GA_FG_DEV static inline
#endif

namespace d3ga {

constexpr float kFgMaxUnit = 17.7f;          // 3 x 5.9
constexpr int kFgCells = 25, kFgCellW = 6;   // the width rule: 25 cells of 6 units
constexpr int kFgSlotLen = 6;                // strlen("{:.3f}")

// a panel as the launch carries it: the caller's d3ga_grid_panel plus what the host derives once
struct FgPanel {
    const float *src;
    const float *value;
    int64_t sc, sh, sw;
    int32_t C, h, w, y0, x0;
    int32_t flags, len, X;
    float color[3];
    int32_t slot;        // byte offset of "{:.3f}" in label, -1: none
    float unit;
    int32_t baseline;    // rows below the panel's top
    uint8_t label[D3GA_GRID_MAX_LABEL];
};

struct FgGrid {
    int32_t n, out_H, out_W, mode, channels, flags;
    float pad;
    int32_t reserved;
    int64_t pitch;
    FgPanel p[D3GA_GRID_MAX_PANELS];
};

// ---- layout ------------------------------------------------------------------------------------------------------------------
D3GA_FHD float fg_unit(int w) {
    float u = (float)w / 150.0f;
    if ((double)u * 150.0 > (double)w) {         // the division rounded up: one float32 down, so that 25 cells do fit
        uint32_t b;
        memcpy(&b, &u, 4);
        b -= 1u;
        memcpy(&u, &b, 4);
    }
    return u > kFgMaxUnit ? kFgMaxUnit : u;
}

D3GA_FHD int fg_baseline(float u, int h, int bottom) { return bottom ? h - (int)(5.0f * u) : (int)(10.0f * u); }

// ---- quantisers --------------------------------------------------------------------------------------------------------------
D3GA_FHD uint8_t fg_quant_save_image(float x) {
    float t = x * 255.0f;
    t = t + 0.5f;
    if (!(t > 0.0f)) return 0;                   // negatives, -0, NaN
    return (uint8_t)(t > 255.0f ? 255.0f : t);
}

D3GA_FHD uint8_t fg_quant_clip(float x) {
    const float t = x * 255.0f;
    if (!(t > 0.0f)) return 0;
    return (uint8_t)(t > 255.0f ? 255.0f : t);
}

D3GA_FHD uint8_t fg_quant(int mode, float x) { return mode == D3GA_GRID_OUT_U8_CLIP ? fg_quant_clip(x) : fg_quant_save_image(x); }

// ---- "{:.3f}" ----------------------------------------------------------------------------------------------------------------
struct FgNum {
    uint32_t q;          // rint(|x| * 1000), at most 999999999
    int32_t kind;        // 0 finite, 1 nan, 2 inf
    int32_t neg;         // a '-' in front (never for nan)
    int32_t n_int;       // integer digits
};

D3GA_FHD FgNum fg_format(float x) {
    FgNum f;
    f.q = 0;
    f.n_int = 1;
    f.neg = __builtin_signbit(x) ? 1 : 0;
    if (x != x) {
        f.kind = 1;
        f.neg = 0;
    } else if (__builtin_isinf(x)) {
        f.kind = 2;
    } else {
        f.kind = 0;
        double r = rint(fabs((double)x) * 1000.0);
        if (r > 999999999.0) r = 999999999.0;
        f.q = (uint32_t)r;
        for (uint32_t i = f.q / 1000u; i >= 10u; i /= 10u) ++f.n_int;
    }
    return f;
}

D3GA_FHD int fg_num_len(const FgNum &f) { return f.neg + (f.kind ? 3 : f.n_int + 4); }

// character i < fg_num_len(f) of the formatted number
D3GA_FHD int fg_num_char(const FgNum &f, int i) {
    if (f.neg) {
        if (i == 0) return '-';
        --i;
    }
    if (f.kind == 1) return i == 0 ? 'n' : (i == 1 ? 'a' : 'n');
    if (f.kind == 2) return i == 0 ? 'i' : (i == 1 ? 'n' : 'f');
    if (i == f.n_int) return '.';
    const int p = i < f.n_int ? 3 + f.n_int - 1 - i : 2 - (i - f.n_int - 1);      // the power of ten of this digit in q
    uint32_t d = f.q;
    for (int k = 0; k < p; ++k) d /= 10u;
    return '0' + (int)(d % 10u);
}

// characters of the label once the slot is filled
D3GA_FHD int fg_label_len(const FgPanel &p, int numlen) { return p.slot < 0 ? p.len : p.len - kFgSlotLen + numlen; }

// character k of it, -1 outside; bytes outside 32..126 are '?'
D3GA_FHD int fg_label_char(const FgPanel &p, const FgNum &num, int numlen, int k) {
    if (k < 0) return -1;
    int j = k;
    if (p.slot >= 0 && k >= p.slot) {
        if (k < p.slot + numlen) return fg_num_char(num, k - p.slot);
        j = k - numlen + kFgSlotLen;
    }
    if (j >= p.len) return -1;
    const int c = p.label[j];
    return (c < 32 || c > 126) ? '?' : c;
}

// ---- coverage ----------------------------------------------------------------------------------------------------------------
// texels (G, r) and (G, r + 1) of the line bitmap in bits 0 and 1: one character lookup for the column
D3GA_FG_DEV int fg_column(const FgPanel &p, const FgNum &num, int numlen, int G, int r) {
    if (G < 0) return 0;
    const int cell = G / kFgCellW, col = G - kFgCellW * cell;
    if (col >= kFgGlyphCols) return 0;
    const int c = fg_label_char(p, num, numlen, cell);
    if (c < 0) return 0;
    const int shift = kFgGlyphCols - 1 - col;
    const int top = (r >= 0 && r < kFgGlyphRows) ? (kFgFont[c - kFgFirstChar][r] >> shift) & 1 : 0;
    const int bot = (r + 1 >= 0 && r + 1 < kFgGlyphRows) ? (kFgFont[c - kFgFirstChar][r + 1] >> shift) & 1 : 0;
    return top | (bot << 1);
}

// the row's coordinate in the line bitmap minus the half texel: text reaches the row iff -1 < fy < 7
D3GA_FHD float fg_row_coord(const FgPanel &p, int ly) {
    const float top = (float)p.baseline - 7.0f * p.unit;
    return ((float)ly + 0.5f - top) / p.unit - 0.5f;
}
D3GA_FHD bool fg_row_has_text(const FgPanel &p, float fy) { return p.len > 0 && fy > -1.0f && fy < 7.0f; }

// bilinear sample at (fx + 0.5, fy + 0.5) units, fy inside (-1, 7); chars = fg_label_len: columns from 6 chars on are empty
D3GA_FG_DEV float fg_sample(const FgPanel &p, const FgNum &num, int numlen, int chars, float fx, float fy) {
    if (!(fx > -1.0f) || !(fx < (float)(kFgCellW * chars))) return 0.0f;
    const float xf = floorf(fx), yf = floorf(fy);
    const float tx = fx - xf, ty = fy - yf;
    const int G = (int)xf, r = (int)yf;
    const int left = fg_column(p, num, numlen, G, r), right = fg_column(p, num, numlen, G + 1, r);
    const float b00 = (float)(left & 1), b01 = (float)(right & 1), b10 = (float)(left >> 1), b11 = (float)(right >> 1);
    const float top = (1.0f - tx) * b00 + tx * b01;
    const float bot = (1.0f - tx) * b10 + tx * b11;
    const float a = (1.0f - ty) * top + ty * bot;
    return a > 1.0f ? 1.0f : a;
}

// coverage of pixel column lx of a row with coordinate fy
D3GA_FG_DEV float fg_alpha(const FgPanel &p, const FgNum &num, int numlen, float fy, int lx) {
    const float gx = ((float)lx + 0.5f - (float)p.X) / p.unit;
    const int chars = fg_label_len(p, numlen);
    float a = fg_sample(p, num, numlen, chars, gx - 0.5f, fy);
    if (p.flags & D3GA_PANEL_BOLD) {
        const float b = fg_sample(p, num, numlen, chars, (gx - 0.5f) - 0.5f, fy);
        a = b > a ? b : a;
    }
    return a;
}

D3GA_FHD float fg_blend(float x, float a, float colour) { return a > 0.0f ? (1.0f - a) * x + a * colour : x; }

// ---- a pixel -----------------------------------------------------------------------------------------------------------------
// the panel that covers canvas pixel (y, x), -1: padding
D3GA_FHD int fg_find_panel(const FgGrid &g, int y, int x) {
    for (int i = 0; i < g.n; ++i) {
        const FgPanel &p = g.p[i];
        if (y >= p.y0 && y < p.y0 + p.h && x >= p.x0 && x < p.x0 + p.w) return i;
    }
    return -1;
}

// the value cell of a row that has text (nothing is read where there is no slot)
D3GA_FHD FgNum fg_row_number(const FgPanel &p) { return p.slot >= 0 ? fg_format(p.value[0]) : fg_format(0.0f); }

// R, G, B, A of canvas pixel (y, x) before the channel order and the quantiser
D3GA_FG_DEV void fg_pixel(const FgGrid &g, int y, int x, float o[4]) {
    const int i = fg_find_panel(g, y, x);
    if (i < 0) {
        o[0] = o[1] = o[2] = o[3] = g.pad;
        return;
    }
    const FgPanel &p = g.p[i];
    const int ly = y - p.y0, lx = x - p.x0;
    const float *s = p.src + (int64_t)ly * p.sh + (int64_t)lx * p.sw;
    o[0] = s[0];
    o[1] = p.C == 1 ? o[0] : s[p.sc];
    o[2] = p.C == 1 ? o[0] : s[2 * p.sc];
    o[3] = p.C == 4 ? s[3 * p.sc] : 1.0f;
    const float fy = fg_row_coord(p, ly);
    if (fg_row_has_text(p, fy)) {
        const FgNum num = fg_row_number(p);
        const float a = fg_alpha(p, num, fg_num_len(num), fy, lx);
        for (int c = 0; c < 3; ++c) o[c] = fg_blend(o[c], a, p.color[c]);
    }
}

// o = R, G, B, A of canvas pixel (y, x) into `out` in the grid's mode: the colour channels swap ends under D3GA_GRID_BGR
D3GA_FHD void fg_store_pixel(const FgGrid &g, void *out, int y, int x, const float o[4]) {
    const bool bgr = g.flags & D3GA_GRID_BGR, four = g.channels == 4;
    const float c0 = bgr ? o[2] : o[0], c2 = bgr ? o[0] : o[2];
    if (g.mode == D3GA_GRID_OUT_F32_CHW) {
        float *f = (float *)out + (int64_t)y * g.out_W + x;
        const int64_t plane = (int64_t)g.out_H * g.out_W;
        f[0] = c0;
        f[plane] = o[1];
        f[2 * plane] = c2;
        if (four) f[3 * plane] = o[3];
    } else if (g.mode == D3GA_GRID_OUT_F32_HWC) {
        float *f = (float *)out + ((int64_t)y * g.out_W + x) * g.channels;
        f[0] = c0;
        f[1] = o[1];
        f[2] = c2;
        if (four) f[3] = o[3];
    } else {
        uint8_t *b = (uint8_t *)out + (int64_t)y * g.pitch + (int64_t)x * g.channels;
        b[0] = fg_quant(g.mode, c0);
        b[1] = fg_quant(g.mode, o[1]);
        b[2] = fg_quant(g.mode, c2);
        if (four) b[3] = fg_quant(g.mode, o[3]);
    }
}

// ---- the host's plan ---------------------------------------------------------------------------------------------------------
// the caller's table, checked, into the launch's; *path = 1: four pixels per thread
static inline int fg_plan(const d3ga_grid_desc *d, const void *out, FgGrid *g, int32_t *path) {
    if (!d || !out) return D3GA_E_NULL;
    if (d->n_panels < 1 || d->n_panels > D3GA_GRID_MAX_PANELS) return D3GA_E_SIZE;
    if (d->out_H < 1 || d->out_W < 1 || d->out_H > D3GA_GRID_MAX_SIDE || d->out_W > D3GA_GRID_MAX_SIDE) return D3GA_E_SIZE;
    if (d->mode < D3GA_GRID_OUT_F32_CHW || d->mode > D3GA_GRID_OUT_U8_CLIP) return D3GA_E_CONFIG;
    if (d->channels != 3 && d->channels != 4) return D3GA_E_CONFIG;
    if (d->flags & ~(D3GA_GRID_BGR | D3GA_GRID_FORCE_SCALAR)) return D3GA_E_CONFIG;
    const bool u8 = d->mode >= D3GA_GRID_OUT_U8_SAVE_IMAGE;
    if (u8 && d->pitch < (int64_t)d->out_W * d->channels) return D3GA_E_SIZE;
    memset(g, 0, sizeof(*g));
    g->n = d->n_panels; g->out_H = d->out_H; g->out_W = d->out_W; g->mode = d->mode; g->channels = d->channels;
    g->flags = d->flags; g->pad = d->pad_value; g->pitch = u8 ? d->pitch : 0;
    bool vec = !(d->flags & D3GA_GRID_FORCE_SCALAR) && d->out_W % 4 == 0;
    vec = vec && (u8 ? (((uintptr_t)out & 3) == 0 && d->pitch % 4 == 0) : ((uintptr_t)out & 15) == 0);
    for (int i = 0; i < d->n_panels; ++i) {
        const d3ga_grid_panel &s = d->panel[i];
        FgPanel &p = g->p[i];
        if (!s.src) return D3GA_E_NULL;
        if (s.C != 1 && s.C != 3 && s.C != 4) return D3GA_E_CONFIG;
        if (s.h < 1 || s.w < 1 || s.y0 < 0 || s.x0 < 0 || s.h > d->out_H - s.y0 || s.w > d->out_W - s.x0) return D3GA_E_SIZE;
        if (s.sc < 0 || s.sh < 0 || s.sw < 0) return D3GA_E_SIZE;
        if (s.label_len < 0 || s.label_len > D3GA_GRID_MAX_LABEL) return D3GA_E_SIZE;
        if (s.flags & ~(D3GA_PANEL_BOTTOM | D3GA_PANEL_BOLD)) return D3GA_E_CONFIG;
        p.src = s.src; p.value = s.value; p.sc = s.sc; p.sh = s.sh; p.sw = s.sw;
        p.C = s.C; p.h = s.h; p.w = s.w; p.y0 = s.y0; p.x0 = s.x0; p.flags = s.flags; p.len = s.label_len; p.X = s.X;
        for (int c = 0; c < 3; ++c) p.color[c] = s.color[c];
        memcpy(p.label, s.label, (size_t)s.label_len);
        p.slot = -1;
        for (int k = 0; k + kFgSlotLen <= s.label_len; ++k)
            if (memcmp(s.label + k, "{:.3f}", kFgSlotLen) == 0) {
                if (p.slot >= 0) return D3GA_E_CONFIG;
                p.slot = k;
            }
        if ((p.slot >= 0) != (s.value != nullptr)) return D3GA_E_CONFIG;
        p.unit = fg_unit(s.w);
        p.baseline = fg_baseline(p.unit, s.h, s.flags & D3GA_PANEL_BOTTOM);
        for (int j = 0; j < i; ++j) {
            const d3ga_grid_panel &t = d->panel[j];
            if (s.y0 < t.y0 + t.h && t.y0 < s.y0 + s.h && s.x0 < t.x0 + t.w && t.x0 < s.x0 + s.w) return D3GA_E_CONFIG;
        }
        vec = vec && s.x0 % 4 == 0 && s.w % 4 == 0 && s.sw == 1 && ((uintptr_t)s.src & 15) == 0 && s.sh % 4 == 0 &&
              (s.C == 1 || s.sc % 4 == 0);
    }
    if (path) *path = vec ? 1 : 0;
    return 0;
}

}  // namespace d3ga
