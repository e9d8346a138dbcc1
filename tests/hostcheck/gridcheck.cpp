// CPU build of d3ga_amd/csrc/frame_grid_math.h: the plan, the per-pixel text of frame_grid.hip's scalar kernel, the quantisers,
// the "{:.3f}" formatter and the font table.  Built by tests/frame_grid_ref.py (g++ -ffp-contract=off).
#include "../../d3ga_amd/csrc/frame_grid_math.h"

using namespace d3ga;

extern "C" {

void hc_grid_quant(int mode, const float *x, int64_t n, uint8_t *out) {
    for (int64_t i = 0; i < n; ++i) out[i] = fg_quant(mode, x[i]);
}

// the formatted number into buf (>= 16 bytes) -> its length
int hc_grid_format(float x, char *buf) {
    const FgNum f = fg_format(x);
    const int n = fg_num_len(f);
    for (int i = 0; i < n; ++i) buf[i] = (char)fg_num_char(f, i);
    return n;
}

void hc_grid_font(uint8_t *out) {
    for (int g = 0; g < kFgGlyphs; ++g)
        for (int r = 0; r < kFgGlyphRows; ++r) out[g * kFgGlyphRows + r] = kFgFont[g][r];
}

float hc_grid_unit(int w) { return fg_unit(w); }
int hc_grid_baseline(float u, int h, int bottom) { return fg_baseline(u, h, bottom); }
float hc_grid_blend(float x, float a, float colour) { return fg_blend(x, a, colour); }

// the label of panel 0 once its slot is filled (buf >= 80 bytes) -> its length
int hc_grid_label(const d3ga_grid_desc *desc, const void *out, char *buf) {
    FgGrid g;
    if (fg_plan(desc, out, &g, nullptr) != 0) return -1;
    const FgNum num = fg_row_number(g.p[0]);
    const int numlen = fg_num_len(num), n = fg_label_len(g.p[0], numlen);
    for (int k = 0; k < n; ++k) buf[k] = (char)fg_label_char(g.p[0], num, numlen, k);
    return fg_label_char(g.p[0], num, numlen, n) == -1 ? n : -2;
}

// coverage of every pixel of panel 0 -> alpha (h, w); the panel's value pointer is host memory here
int hc_grid_alpha(const d3ga_grid_desc *desc, const void *out, float *alpha) {
    FgGrid g;
    const int st = fg_plan(desc, out, &g, nullptr);
    if (st != 0) return st;
    const FgPanel &p = g.p[0];
    for (int ly = 0; ly < p.h; ++ly) {
        const float fy = fg_row_coord(p, ly);
        const bool text = fg_row_has_text(p, fy);
        const FgNum num = text ? fg_row_number(p) : fg_format(0.0f);
        for (int lx = 0; lx < p.w; ++lx) alpha[(size_t)ly * p.w + lx] = text ? fg_alpha(p, num, fg_num_len(num), fy, lx) : 0.0f;
    }
    return 0;
}

// what the launch receives, for the plan tests: unit, baseline and slot of every panel
int hc_grid_plan(const d3ga_grid_desc *desc, const void *out, int32_t *path, float *unit, int32_t *baseline, int32_t *slot) {
    FgGrid g;
    const int st = fg_plan(desc, out, &g, path);
    if (st != 0) return st;
    for (int i = 0; i < g.n; ++i) {
        unit[i] = g.p[i].unit;
        baseline[i] = g.p[i].baseline;
        slot[i] = g.p[i].slot;
    }
    return 0;
}

// frame_grid_scalar_kernel, a pixel after the other; every pointer of desc is host memory
int hc_grid_compose(const d3ga_grid_desc *desc, void *out, int32_t *path) {
    FgGrid g;
    const int st = fg_plan(desc, out, &g, path);
    if (st != 0) return st;
    for (int y = 0; y < g.out_H; ++y)
        for (int x = 0; x < g.out_W; ++x) {
            float o[4];
            fg_pixel(g, y, x, o);
            fg_store_pixel(g, out, y, x, o);
        }
    return 0;
}
}
