// CPU build of d3ga_amd/csrc/point_raster_math.h: the loops of point_raster.hip (points -> tiles -> lists, tile -> pixels -> the
// K-slot insertion, the composite gather) around the header's own per-element functions.  Same arguments as the d3ga_points_*
// entry points (include/d3ga.h), host memory.  Built by tests/point_ref.py::host_lib (g++ -ffp-contract=off).
#include <vector>

#include "../../d3ga_amd/csrc/point_raster_math.h"

using namespace d3ga;

template <int K>
static void tile_pixels(const std::vector<PointRec> &list, int tx, int ty, int H, int W, float s2, float r2, int64_t b, int32_t *idx,
                        float *zbuf, float *dists) {
    for (int lane = 0; lane < kPointTile * kPointTile; ++lane) {
        const int i = tx * kPointTile + (lane & (kPointTile - 1)), j = ty * kPointTile + (lane >> 4);
        if (i >= W || j >= H) continue;
        uint64_t key[K];
        float d2[K];
        for (int k = 0; k < K; ++k) { key[k] = kPointEmptyKey; d2[k] = -1.f; }
        for (const PointRec &r : list) point_visit<K>(r, i, j, s2, r2, key, d2);
        const int64_t p = ((b * H + j) * W + i) * K;
        for (int k = 0; k < K; ++k) {
            const bool filled = key[k] != kPointEmptyKey;
            idx[p + k] = filled ? (int32_t)(uint32_t)key[k] : -1;
            if (zbuf) zbuf[p + k] = filled ? point_key_depth(key[k]) : -1.f;
            if (dists) dists[p + k] = filled ? d2[k] : -1.f;
        }
    }
}

extern "C" {

// -> the length of the longest tile list, or < 0 (a point that touches more tiles than point_tiles_per_axis allows: -1)
// reversed != 0: the lists are filled from the last point to the first (the result must not depend on it)
int64_t hc_points_rasterize(int B, int P, int H, int W, int K, float radius, const float *points, const float *cams, int reversed,
                            int32_t *idx, float *zbuf, float *dists) {
    const int tiles_x = (W + kPointTile - 1) / kPointTile, tiles_y = (H + kPointTile - 1) / kPointTile;
    const float r_px = point_radius_px(radius, H, W), s2 = point_ndc_scale2(H, W), r2 = radius * radius;
    const int64_t per_axis = point_tiles_per_axis(r_px);
    int64_t longest = 0;
    for (int64_t b = 0; b < B; ++b) {
        std::vector<std::vector<PointRec>> lists((size_t)tiles_x * tiles_y);
        for (int q = 0; q < P; ++q) {
            const int p = reversed ? P - 1 - q : q;
            PointRec r;
            int tx0, ty0, tx1, ty1;
            if (!point_setup(cams + kMeshCam * b, points + 3 * (b * P + p), (uint32_t)p, H, W, r_px, &r, &tx0, &ty0, &tx1, &ty1)) continue;
            if (tx1 - tx0 + 1 > per_axis || ty1 - ty0 + 1 > per_axis) return -1;
            for (int ty = ty0; ty <= ty1; ++ty)
                for (int tx = tx0; tx <= tx1; ++tx) lists[(size_t)ty * tiles_x + tx].push_back(r);
        }
        for (int ty = 0; ty < tiles_y; ++ty)
            for (int tx = 0; tx < tiles_x; ++tx) {
                const std::vector<PointRec> &list = lists[(size_t)ty * tiles_x + tx];
                if ((int64_t)list.size() > longest) longest = (int64_t)list.size();
                switch (K) {
                    case 1: tile_pixels<1>(list, tx, ty, H, W, s2, r2, b, idx, zbuf, dists); break;
                    case 2: tile_pixels<2>(list, tx, ty, H, W, s2, r2, b, idx, zbuf, dists); break;
                    case 3: tile_pixels<3>(list, tx, ty, H, W, s2, r2, b, idx, zbuf, dists); break;
                    case 4: tile_pixels<4>(list, tx, ty, H, W, s2, r2, b, idx, zbuf, dists); break;
                    case 5: tile_pixels<5>(list, tx, ty, H, W, s2, r2, b, idx, zbuf, dists); break;
                    case 6: tile_pixels<6>(list, tx, ty, H, W, s2, r2, b, idx, zbuf, dists); break;
                    case 7: tile_pixels<7>(list, tx, ty, H, W, s2, r2, b, idx, zbuf, dists); break;
                    case 8: tile_pixels<8>(list, tx, ty, H, W, s2, r2, b, idx, zbuf, dists); break;
                    default: return -2;
                }
            }
    }
    return longest;
}

// every (pixel, point) pair through the plain membership test, no box and no tiles: what the box must not change
int64_t hc_points_members_plain(int B, int P, int H, int W, float radius, const float *points, const float *cams) {
    const float s2 = point_ndc_scale2(H, W), r2 = radius * radius;
    int64_t n = 0;
    for (int64_t b = 0; b < B; ++b)
        for (int p = 0; p < P; ++p) {
            PointRec r;
            int t[4];
            // a box as wide as the frame: only the drop rule is left of the setup
            if (!point_setup(cams + kMeshCam * b, points + 3 * (b * P + p), (uint32_t)p, H, W, 1.0e9f, &r, t, t + 1, t + 2, t + 3)) continue;
            for (int j = 0; j < H; ++j)
                for (int i = 0; i < W; ++i) n += point_dist2(r, i, j, s2) < r2 ? 1 : 0;
        }
    return n;
}

// the members the tiled path sees: what hc_points_rasterize would count with K unbounded
int64_t hc_points_members_tiled(int B, int P, int H, int W, float radius, const float *points, const float *cams) {
    const float r_px = point_radius_px(radius, H, W), s2 = point_ndc_scale2(H, W), r2 = radius * radius;
    int64_t n = 0;
    for (int64_t b = 0; b < B; ++b)
        for (int p = 0; p < P; ++p) {
            PointRec r;
            int tx0, ty0, tx1, ty1;
            if (!point_setup(cams + kMeshCam * b, points + 3 * (b * P + p), (uint32_t)p, H, W, r_px, &r, &tx0, &ty0, &tx1, &ty1)) continue;
            for (int j = ty0 * kPointTile; j < (ty1 + 1) * kPointTile && j < H; ++j)
                for (int i = tx0 * kPointTile; i < (tx1 + 1) * kPointTile && i < W; ++i) n += point_dist2(r, i, j, s2) < r2 ? 1 : 0;
        }
    return n;
}

void hc_points_composite(int B, int P, int H, int W, int K, float radius, const int32_t *idx, const float *dists, const float *colors,
                         const float *bg, float *image) {
    const float r2 = radius * radius;
    for (int64_t b = 0; b < B; ++b)
        for (int64_t q = 0; q < (int64_t)H * W; ++q) {
            const int64_t p = b * H * W + q;
            point_composite(K, P, idx + p * K, dists + p * K, r2, colors ? colors + 3 * b * P : nullptr, bg, image + 3 * p);
        }
}
}
