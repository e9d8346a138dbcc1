// point_raster_math.h -- the per-element arithmetic of the point-cloud rasterizer and compositor (point_raster.hip): the
// projection and the drop rule, the box of pixel centres a disc can reach and the tiles it touches, the squared NDC distance,
// the (depth, index) key, the K-slot insertion and pytorch3d's AlphaCompositor as the reference's recorder/pc_renderer.py uses
// it.  Semantics: DESIGN.md 4.4h (specification of record).  Compiles for the host as it is (tests/hostcheck/pointcheck.cpp
// runs this very text on the CPU against tests/point_ref.py); point_raster.hip is compiled with -ffp-contract=off and
// correctly rounded division, so the device evaluates every expression here as g++ does.
#pragma once
#include "mesh_raster_math.h"

namespace d3ga {

constexpr int kPointTile = 16;                  // pixels per side of a tile: one 256-lane workgroup, one lane per pixel
constexpr int kPointMaxK = D3GA_POINTS_MAX_K;   // points kept per pixel, at most
constexpr float kPointNear = kMeshNear;         // a point at z <= this is dropped
constexpr uint64_t kPointEmptyKey = ~(uint64_t)0;
constexpr float kPointDefaultR = 154.f / 255.f, kPointDefaultG = 205.f / 255.f, kPointDefaultB = 50.f / 255.f;

// What the tile kernel needs of a point: 16 bytes.
struct alignas(16) PointRec {
    float u, v, z;                              // screen position in pixels, view depth
    uint32_t index;                             // of the point within its cloud
};

// the radius in pixels: NDC spans [-1, 1] over the shorter side
D3GA_FHD float point_radius_px(float radius, int H, int W) { return radius * (float)(H < W ? H : W) / 2.f; }
// (2 / min(H, W))^2: squared pixels -> squared NDC units
D3GA_FHD float point_ndc_scale2(int H, int W) {
    const float s = 2.f / (float)(H < W ? H : W);
    return s * s;
}

// The box is cut from r_px with this slack, so that no float32 rounding of the box can exclude a pixel that passes the
// membership test (which alone decides): the test bounds |dx| by r_px (1 + a few ulp), the box bounds suffer ulp(u) <= 0.002
// inside the largest frame.
D3GA_FHD float point_box_radius(float r_px) { return r_px * 1.001f + 0.01f; }

// Tiles per axis a box can span at most: it holds at most floor(2 r_box) + 2 pixel centres (one more than the exact count
// for the rounding of its two ends), and n consecutive pixels touch at most floor((n + 14) / 16) + 1 tiles.
static inline int64_t point_tiles_per_axis(float r_px) {
    float rb = point_box_radius(r_px);
    if (!(rb <= 65536.f)) rb = 65536.f;         // wider than any frame (and NaN)
    const int64_t n = (int64_t)floorf(2.f * rb) + 2;
    return (n + 14) / kPointTile + 1;
}

// Project a point; -> the number of tiles its box touches (0: dropped: z <= 0.01, anything not finite, or a box that holds no
// pixel centre of the frame), the record and the tile rectangle [tx0, tx1] x [ty0, ty1].
D3GA_FHD int point_setup(const float *cam, const float *x, uint32_t index, int H, int W, float r_px, PointRec *r, int *tx0, int *ty0,
                         int *tx1, int *ty1) {
    float v[3];
    mesh_view(cam, x, v);
    if (!(v[2] > kPointNear) || !(v[2] <= 3.0e38f)) return 0;
    r->u = cam[12] * v[0] / v[2] + cam[14];
    r->v = cam[13] * v[1] / v[2] + cam[15];
    r->z = v[2];
    r->index = index;
    // pixel i samples i + 0.5: the columns with u - r - 0.5 <= i <= u + r - 0.5
    const float rb = point_box_radius(r_px);
    int i0 = mesh_clamp_index(ceilf((r->u - rb) - 0.5f), W), i1 = mesh_clamp_index(floorf((r->u + rb) - 0.5f), W);
    int j0 = mesh_clamp_index(ceilf((r->v - rb) - 0.5f), H), j1 = mesh_clamp_index(floorf((r->v + rb) - 0.5f), H);
    if (i0 < 0) i0 = 0;
    if (j0 < 0) j0 = 0;
    if (i1 > W - 1) i1 = W - 1;
    if (j1 > H - 1) j1 = H - 1;
    if (i0 > i1 || j0 > j1) return 0;
    *tx0 = i0 / kPointTile; *tx1 = i1 / kPointTile;
    *ty0 = j0 / kPointTile; *ty1 = j1 / kPointTile;
    return (*tx1 - *tx0 + 1) * (*ty1 - *ty0 + 1);
}

// squared NDC distance of pixel (i, j)'s centre from the point
D3GA_FHD float point_dist2(const PointRec &r, int i, int j, float s2) {
    const float dx = ((float)i + 0.5f) - r.u, dy = ((float)j + 0.5f) - r.v;
    return (dx * dx + dy * dy) * s2;
}

// Can no pixel centre of the four rows first_row .. first_row + 3 belong to the point?  Conservative by the box's slack: a member
// has |v - (j + 0.5)| < r_px (1 + a few ulp), and the rows' centres lie within 1.5 of first_row + 2.
D3GA_FHD bool point_rows_miss(const PointRec &r, int first_row, float r_px) {
    return fabsf(r.v - ((float)first_row + 2.f)) > point_box_radius(r_px) + 1.5f;
}

// float_bits(z) << 32 | index: z > 0, so keys order by depth and, among equal depths, by index: a total order, whatever the
// order in which the points arrive
D3GA_FHD uint64_t point_key(const PointRec &r) { return ((uint64_t)mesh_float_bits(r.z) << 32) | r.index; }

D3GA_FHD float point_key_depth(uint64_t key) {
    const uint32_t u = (uint32_t)(key >> 32);
    float z;
    __builtin_memcpy(&z, &u, 4);
    return z;
}

// keep the K smallest keys, ascending, with their dist2 (key[k] = kPointEmptyKey: slot k is empty)
template <int K>
D3GA_FHD void point_insert(uint64_t *key, float *d2, uint64_t k, float d) {
    if (!(k < key[K - 1])) return;
    key[K - 1] = k;
    d2[K - 1] = d;
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int s = K - 1; s > 0; --s) {
        const bool sw = key[s] < key[s - 1];
        const uint64_t a = key[s - 1], b = key[s];
        const float da = d2[s - 1], db = d2[s];
        key[s - 1] = sw ? b : a; key[s] = sw ? a : b;
        d2[s - 1] = sw ? db : da; d2[s] = sw ? da : db;
    }
}

// one point against one pixel: the membership test (strict) and the insertion
template <int K>
D3GA_FHD void point_visit(const PointRec &r, int i, int j, float s2, float r2, uint64_t *key, float *d2) {
    const float d = point_dist2(r, i, j, s2);
    if (d < r2) point_insert<K>(key, d2, point_key(r), d);
}

// AlphaCompositor over a pixel's K fragments, front to back: w_k = 1 - dist2_k / radius^2, colour = sum_k w_k f_k prod_{j<k}
// (1 - w_j); the background only where slot 0 is empty (a covered pixel is NOT blended with it).  colors: the cloud's (P,3)
// colours, null: the reference's default.
D3GA_FHD void point_composite(int K, int P, const int32_t *idx, const float *dists, float r2, const float *colors, const float *bg,
                              float *rgb) {
    if ((uint32_t)idx[0] >= (uint32_t)P) {
        rgb[0] = bg[0]; rgb[1] = bg[1]; rgb[2] = bg[2];
        return;
    }
    float T = 1.f, acc[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < K; ++k) {
        if ((uint32_t)idx[k] >= (uint32_t)P) break;
        const float w = 1.f - dists[k] / r2, wt = w * T;
        const float *f = colors ? colors + 3 * (int64_t)idx[k] : nullptr;
        acc[0] = acc[0] + wt * (f ? f[0] : kPointDefaultR);
        acc[1] = acc[1] + wt * (f ? f[1] : kPointDefaultG);
        acc[2] = acc[2] + wt * (f ? f[2] : kPointDefaultB);
        T = T * (1.f - w);
    }
    rgb[0] = acc[0]; rgb[1] = acc[1]; rgb[2] = acc[2];
}

}  // namespace d3ga
