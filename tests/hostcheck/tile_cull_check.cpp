// tile_cull_check.cpp -- TEST-ONLY, stand-alone (no GPU): d3ga_math.h's tile_rect_tight -- the rectangle binning uses under
// d3ga_raster_params::tile_cull -- against a float64 brute force over integer pixels.  For every case (centre, half extents of the
// alpha >= 1/255 box, reference rectangle from tile_rect):
//   1. the tight rectangle lies inside the reference rectangle;
//   2. it is not empty (the reference rectangle of a visible splat never is);
//   3. no tile of the reference rectangle that holds an integer pixel (x, y) with |x - px| <= hx and |y - py| <= hy (float64) is
//      dropped;
//   4. unless the one-tile fallback was taken, every kept tile passes the float32 test it was derived from,
//      !(c + h < 16 t) && !(c - h > 16 t + 15) on both axes, and no tile of the reference rectangle outside it does.
// Prints one line per group of cases, "<group> cases=<n> ok", and returns the number of failed cases (0 = all good).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>

#include "../../d3ga_amd/csrc/d3ga_math.h"

using namespace d3ga;

static int g_fail = 0;

static bool axis_has_pixel(int t, double c, double h) {          // float64, pixel by pixel
    if (!(h >= 0.0)) return false;
    for (int x = kTile * t; x < kTile * t + kTile; ++x)
        if (c - h <= (double)x && (double)x <= c + h) return true;
    return false;
}
static bool axis_passes_f32(int t, float c, float h) {           // the forward's stage-one expression, the tile's two quadrants merged
    const float lo = c - h, hi = c + h;
    return !(hi < (float)(kTile * t)) && !(lo > (float)(kTile * t + kTile - 1));
}

static bool check(const char *what, float px, float py, float hx, float hy, const int ref[4]) {
    int out[4] = {-7, -7, -7, -7};
    tile_rect_tight(ref, px, py, hx, hy, out);
    bool ok = true;
    auto fail = [&](const char *why) {
        if (ok) fprintf(stderr, "%s: %s  centre (%.9g, %.9g) extents (%.9g, %.9g) ref [%d %d %d %d] tight [%d %d %d %d]\n", what, why,
                        (double)px, (double)py, (double)hx, (double)hy, ref[0], ref[1], ref[2], ref[3], out[0], out[1], out[2], out[3]);
        ok = false;
    };
    if (out[0] < ref[0] || out[1] < ref[1] || out[2] > ref[2] || out[3] > ref[3]) fail("larger than the reference rectangle");
    if (out[2] <= out[0] || out[3] <= out[1]) fail("empty");
    bool any_f32 = false;
    for (int ty = ref[1]; ty < ref[3] && ok; ++ty)
        for (int tx = ref[0]; tx < ref[2] && ok; ++tx) {
            const bool kept = tx >= out[0] && tx < out[2] && ty >= out[1] && ty < out[3];
            const bool pixel = !(hx < 0.f) && axis_has_pixel(tx, px, hx) && axis_has_pixel(ty, py, hy);
            if (pixel && !kept) fail("dropped a tile that has a pixel inside the box");
            const bool f32 = !(hx < 0.f) && axis_passes_f32(tx, px, hx) && axis_passes_f32(ty, py, hy);
            any_f32 = any_f32 || f32;
            if (f32 && !kept) fail("dropped a tile the forward's test accepts");
        }
    if (ok && any_f32)                              // not the fallback: nothing kept that the forward's test rejects everywhere
        for (int ty = out[1]; ty < out[3] && ok; ++ty)
            for (int tx = out[0]; tx < out[2] && ok; ++tx)
                if (!(axis_passes_f32(tx, px, hx) && axis_passes_f32(ty, py, hy))) fail("kept a tile the forward's test rejects");
    if (ok && !any_f32 && (out[2] - out[0]) * (out[3] - out[1]) != 1) fail("the fallback is not one tile");
    if (!ok) ++g_fail;
    return ok;
}

// the reference rectangle of a visible splat (project_gaussian: tile_rect, culled when empty)
static bool ref_rect(float px, float py, float radius, int gx, int gy, int ref[4]) {
    tile_rect(px, py, radius, gx, gy, ref);
    return (ref[2] - ref[0]) * (ref[3] - ref[1]) != 0;
}

int main() {
    const int W = 1920, H = 1080, gx = (W + kTile - 1) / kTile, gy = (H + kTile - 1) / kTile;
    int ref[4], n;
    const int before = g_fail;
    auto done = [&](const char *group, int cases, int fail0) { printf("%s cases=%d %s\n", group, cases, g_fail == fail0 ? "ok" : "FAILED"); };

    // ---- box ends exactly on a tile edge (first / last pixel of a tile, and the half pixel beside them) ----
    n = 0;
    for (float edge : {16.f, 32.f, 48.f, 1904.f})
        for (float d : {-1.f, -0.5f, 0.f, 0.5f, 1.f})
            for (float h : {0.f, 3.f, 8.f, 20.f}) {
                // right end on the edge: hi = edge + d;  left end on the last pixel of the tile before: lo = edge - 1 + d
                if (ref_rect(edge + d - h, 100.f, 64.f, gx, gy, ref)) { check("right end on an edge", edge + d - h, 100.f, h, 5.f, ref); ++n; }
                if (ref_rect(edge - 1.f + d + h, 100.f, 64.f, gx, gy, ref)) { check("left end on an edge", edge - 1.f + d + h, 100.f, h, 5.f, ref); ++n; }
                if (ref_rect(100.f, edge + d - h, 64.f, gx, gy, ref)) { check("bottom end on an edge", 100.f, edge + d - h, 5.f, h, ref); ++n; }
                if (ref_rect(100.f, edge - 1.f + d + h, 64.f, gx, gy, ref)) { check("top end on an edge", 100.f, edge - 1.f + d + h, 5.f, h, ref); ++n; }
            }
    done("tile_edges", n, before);

    // ---- centre off-screen with the box reaching in; and not reaching in ----
    int f0 = g_fail; n = 0;
    for (float c : {-20.f, -0.5f, -300.f, (float)W + 10.f, (float)W - 0.5f})
        for (float h : {5.f, 19.5f, 20.f, 30.f, 400.f})
            for (float r : {25.f, 40.f, 500.f}) {
                if (ref_rect(c, 500.f, r, gx, gy, ref)) { check("off-screen x", c, 500.f, h, 12.f, ref); ++n; }
                if (ref_rect(500.f, c * (float)H / (float)W, r, gx, gy, ref)) { check("off-screen y", 500.f, c * (float)H / (float)W, 12.f, h, ref); ++n; }
            }
    done("off_screen", n, f0);

    // ---- hx = -1 (opacity x 255 < 1): stays visible, one tile ----
    f0 = g_fail; n = 0;
    for (float c : {5.f, 15.9f, 16.f, 700.3f, -3.f, (float)W + 3.f})
        for (float r : {4.f, 40.f, 3000.f})
            if (ref_rect(c, 0.5f * c, r, gx, gy, ref)) {
                check("hx = -1", c, 0.5f * c, -1.f, -1.f, ref); ++n;
                int out[4];
                tile_rect_tight(ref, c, 0.5f * c, -1.f, -1.f, out);
                if ((out[2] - out[0]) * (out[3] - out[1]) != 1) { fprintf(stderr, "hx = -1: not one tile\n"); ++g_fail; }
            }
    done("no_alpha", n, f0);

    // ---- a box narrower than one pixel lying between pixel rows / columns ----
    f0 = g_fail; n = 0;
    for (float c : {31.5f, 15.5f, 100.5f, 16.4f, 0.5f, -0.5f})
        for (float h : {0.02f, 0.3f, 0.49f, 0.5f})
        {
            if (ref_rect(200.f, c, 3.f, gx, gy, ref)) { check("between rows", 200.f, c, 6.f, h, ref); ++n; }
            if (ref_rect(c + 64.f, 200.f, 3.f, gx, gy, ref)) { check("between columns", c + 64.f, 200.f, h, 6.f, ref); ++n; }
        }
    done("between_pixels", n, f0);

    // ---- a screen-filling box; extents beyond any raster, infinite, NaN ----
    f0 = g_fail; n = 0;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (float h : {1e4f, 3e9f, 1e30f, inf, nan})
        for (float c : {960.f, -5000.f, 4e9f})
            if (ref_rect(c, 540.f, 1e5f, gx, gy, ref)) {
                check("screen-filling", c, 540.f, h, h, ref); ++n;
                check("screen-filling x", c, 540.f, h, 7.f, ref); ++n;
                check("screen-filling y", 960.f, 540.f, 7.f, h, ref); ++n;
            }
    if (ref_rect(960.f, 540.f, 1e5f, gx, gy, ref)) {
        int out[4];
        tile_rect_tight(ref, 960.f, 540.f, 1e4f, 1e4f, out);
        if (out[0] != 0 || out[1] != 0 || out[2] != gx || out[3] != gy) { fprintf(stderr, "screen-filling: not the whole grid\n"); ++g_fail; }
    }
    done("screen_filling", n, f0);

    // ---- random centres and extents, on rasters whose last tile is partial as well ----
    f0 = g_fail; n = 0;
    std::mt19937 rng(12345);
    std::uniform_real_distribution<float> u(0.f, 1.f);
    const int sizes[3][2] = {{1920, 1080}, {161, 143}, {97, 61}};
    for (int it = 0; it < 60000; ++it) {
        const int w = sizes[it % 3][0], h = sizes[it % 3][1];
        const int tgx = (w + kTile - 1) / kTile, tgy = (h + kTile - 1) / kTile;
        float px = -60.f + u(rng) * ((float)w + 120.f), py = -60.f + u(rng) * ((float)h + 120.f);
        if (it % 7 == 0) px = floorf(px) + (it % 2 ? 0.5f : 0.f);          // centres on pixels and half pixels
        if (it % 11 == 0) py = floorf(py);
        const float radius = ceilf(1.f + 80.f * u(rng) * u(rng));
        float hx = radius * (0.05f + 1.2f * u(rng)), hy = radius * (0.05f + 1.2f * u(rng));
        if (it % 5 == 0) hx = floorf(hx) + 0.5f * (float)(it % 3);         // ends on integers and half integers
        if (it % 13 == 0) hy = 0.6f * u(rng);
        if (!ref_rect(px, py, radius, tgx, tgy, ref)) continue;
        check("random", px, py, hx, hy, ref); ++n;
    }
    done("random", n, f0);
    return g_fail > 255 ? 255 : g_fail;
}
