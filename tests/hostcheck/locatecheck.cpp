// locatecheck.cpp -- csrc/bary_math.h (the arithmetic the kernels of bary.hip run: barycentric weights, the two selection rules,
// the 3-NN insertion, mean and ring search) on the CPU, built with g++ -ffp-contract=off as the device build is: the yardstick
// the GPU results are compared with bit for bit (tests/locate_ref.py loads it as a shared library).  The loops below are the
// kernels' loops: the exhaustive search walks the tets in chunks of kBaryChunk as the LDS staging does.  With -DLOCATECHECK_MAIN
// it is a stand-alone program that runs every entry on a small built-in case; that program is what gets built with
// -fsanitize=address,undefined.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../d3ga_amd/csrc/bary_math.h"

using namespace d3ga;

static V3 load_point(const float *points, int i) { return v3(points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2]); }

extern "C" int hc_compute_bary(int P, int T, const float *points, const float *corners, float *barys, int32_t *tid, uint8_t *active) {
    if (P < 0 || T <= 0) return -2;
    for (int i = 0; i < P; ++i) {
        const V3 p = load_point(points, i);
        BaryBest best;
        bary_best_clear(best, 0);
        for (int base = 0; base < T; base += kBaryChunk) {
            const int cnt = bary_imin(kBaryChunk, T - base);
            bary_scan_chunk(best, p, corners + (size_t)base * 12, base, cnt);
        }
        memcpy(barys + 4 * (size_t)i, best.w, 16);
        tid[i] = best.t;
        active[i] = best.mn >= 0.f ? 1 : 0;
    }
    return 0;
}

// compute_bary_grid_kernel: origin_h = {ox, oy, oz, h}; the kernel receives 1.0f / h
extern "C" int hc_compute_bary_grid(int P, const float *points, const float *corners, const int32_t *cell_start, const int32_t *cell_tets,
                                    const float *origin_h, const int32_t *dims, float *barys, int32_t *tid, float *min_weight) {
    if (P < 0 || dims[0] <= 0 || dims[1] <= 0 || dims[2] <= 0 || !(origin_h[3] > 0.f)) return -2;
    const float ox = origin_h[0], oy = origin_h[1], oz = origin_h[2], inv_h = 1.0f / origin_h[3];
    const int nx = dims[0], ny = dims[1], nz = dims[2];
    for (int i = 0; i < P; ++i) {
        const V3 p = load_point(points, i);
        BaryBest best;
        bary_best_clear(best, kBaryNoTet);
        const int cx = bary_cell(p.x, ox, inv_h), cy = bary_cell(p.y, oy, inv_h), cz = bary_cell(p.z, oz, inv_h);
        if (cx >= 0 && cy >= 0 && cz >= 0 && cx < nx && cy < ny && cz < nz) {
            const int cell = (cz * ny + cy) * nx + cx;
            for (int k = cell_start[cell]; k < cell_start[cell + 1]; ++k) {
                const int t = cell_tets[k];
                bary_select_grid(best, tet_weights(p, corners + 12 * (size_t)t), t);
            }
        }
        memcpy(barys + 4 * (size_t)i, best.w, 16);
        tid[i] = best.t == kBaryNoTet ? 0 : best.t;
        min_weight[i] = best.mn;
    }
    return 0;
}

extern "C" int hc_knn3_mean_dist2(int P, const float *points, float *out) {
    if (P < 0) return -2;
    for (int i = 0; i < P; ++i) {
        const V3 p = load_point(points, i);
        float d0 = INFINITY, d1 = INFINITY, d2 = INFINITY;
        for (int j = 0; j < P; ++j) {
            if (j == i) continue;
            knn3_insert(p, points + 3 * (size_t)j, d0, d1, d2);
        }
        out[i] = knn3_mean(d0, d1, d2);
    }
    return 0;
}

extern "C" int hc_knn3_mean_dist2_grid(int P, const float *points, const int32_t *cell_start, const int32_t *cell_points,
                                       const float *origin_h, const int32_t *dims, float *out) {
    if (P < 0 || dims[0] <= 0 || dims[1] <= 0 || dims[2] <= 0 || !(origin_h[3] > 0.f)) return -2;
    for (int i = 0; i < P; ++i)
        out[i] = knn3_grid_search(i, points, cell_start, cell_points, origin_h[0], origin_h[1], origin_h[2], origin_h[3], dims[0], dims[1],
                                  dims[2]);
    return 0;
}

#ifdef LOCATECHECK_MAIN
static uint32_t rng_state = 2463534242u;
static float uniform() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return (float)(rng_state >> 8) / 16777216.0f;
}

// every item in the cells its inclusive cell box [lo, hi] overlaps, ascending inside a cell
static void csr(const std::vector<int> &lo, const std::vector<int> &hi, const int32_t *dims, std::vector<int32_t> &start,
                std::vector<int32_t> &items) {
    const int n = (int)lo.size() / 3, cells = dims[0] * dims[1] * dims[2];
    std::vector<std::vector<int32_t>> lists(cells);
    for (int t = 0; t < n; ++t)
        for (int z = lo[3 * t + 2]; z <= hi[3 * t + 2]; ++z)
            for (int y = lo[3 * t + 1]; y <= hi[3 * t + 1]; ++y)
                for (int x = lo[3 * t]; x <= hi[3 * t]; ++x) lists[(z * dims[1] + y) * dims[0] + x].push_back(t);
    start.assign(cells + 1, 0);
    items.clear();
    for (int c = 0; c < cells; ++c) {
        items.insert(items.end(), lists[c].begin(), lists[c].end());
        start[c + 1] = (int32_t)items.size();
    }
    if (items.empty()) items.push_back(0);
}

static int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

int main() {
    int failures = 0;
    // a 3 x 3 x 3 lattice of cells of edge 1/2, six Kuhn tets each (T = 162), then as many again translated far off, so that the
    // exhaustive search crosses a chunk boundary; two zero-volume tets at the end
    std::vector<float> corners;
    const int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    for (int rep = 0; rep < 2; ++rep)
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j)
                for (int k = 0; k < 3; ++k)
                    for (const auto &pm : perms) {
                        float c[3] = {0.5f * i + 8.f * rep, 0.5f * j, 0.5f * k};
                        corners.insert(corners.end(), c, c + 3);
                        for (int s = 0; s < 3; ++s) { c[pm[s]] += 0.5f; corners.insert(corners.end(), c, c + 3); }
                    }
    const float flat[2][12] = {{0.f, 0.f, 0.25f, 1.f, 0.f, 0.25f, 0.f, 1.f, 0.25f, 1.f, 1.f, 0.25f},
                               {0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f}};
    corners.insert(corners.end(), flat[0], flat[0] + 12);
    corners.insert(corners.end(), flat[1], flat[1] + 12);
    const int T = (int)corners.size() / 12;
    // queries: lattice points of spacing 1/4 in [-1/4, 7/4]^3 (exact ties, outside points), random ones, and three not finite
    std::vector<float> pts;
    for (int i = -1; i <= 7; ++i)
        for (int j = -1; j <= 7; ++j)
            for (int k = -1; k <= 7; ++k) { pts.push_back(0.25f * i); pts.push_back(0.25f * j); pts.push_back(0.25f * k); }
    for (int i = 0; i < 300; ++i) { pts.push_back(2.f * uniform() - 0.25f + (i % 2 ? 8.f : 0.f)); pts.push_back(2.f * uniform() - 0.25f); pts.push_back(2.f * uniform() - 0.25f); }
    const float bad[3][3] = {{NAN, 0.3f, 0.3f}, {0.3f, INFINITY, 0.3f}, {-INFINITY, -INFINITY, -INFINITY}};
    for (const auto &b : bad) pts.insert(pts.end(), b, b + 3);
    const int P = (int)pts.size() / 3;
    std::vector<float> ba(4 * (size_t)P), bb(4 * (size_t)P), mw(P);
    std::vector<int32_t> ta(P), tb(P);
    std::vector<uint8_t> act(P);
    if (hc_compute_bary(P, T, pts.data(), corners.data(), ba.data(), ta.data(), act.data())) ++failures;
    // the tet grid: cells of edge 1, every tet in the cells its box overlaps
    float lo3[3] = {INFINITY, INFINITY, INFINITY}, hi3[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (size_t v = 0; v < corners.size(); ++v) { lo3[v % 3] = fminf(lo3[v % 3], corners[v]); hi3[v % 3] = fmaxf(hi3[v % 3], corners[v]); }
    const float origin_h[4] = {lo3[0], lo3[1], lo3[2], 1.0f};
    const int32_t dims[3] = {(int)ceilf(hi3[0] - lo3[0]) + 1, (int)ceilf(hi3[1] - lo3[1]) + 1, (int)ceilf(hi3[2] - lo3[2]) + 1};
    std::vector<int> lo(3 * (size_t)T), hi(3 * (size_t)T);
    for (int t = 0; t < T; ++t)
        for (int a = 0; a < 3; ++a) {
            float l = INFINITY, h = -INFINITY;
            for (int c = 0; c < 4; ++c) { l = fminf(l, corners[12 * t + 3 * c + a]); h = fmaxf(h, corners[12 * t + 3 * c + a]); }
            lo[3 * t + a] = clampi((int)floorf(l - origin_h[a]), dims[a] - 1);
            hi[3 * t + a] = clampi((int)floorf(h - origin_h[a]), dims[a] - 1);
        }
    std::vector<int32_t> start, items;
    csr(lo, hi, dims, start, items);
    if (hc_compute_bary_grid(P, pts.data(), corners.data(), start.data(), items.data(), origin_h, dims, bb.data(), tb.data(), mw.data())) ++failures;
    int inside = 0;
    for (int i = 0; i < P; ++i) {
        if (ta[i] >= T - 2) { printf("point %d: a zero-volume tet was chosen\n", i); ++failures; }
        if (i >= P - 3 && (act[i] || ta[i] != 0 || ba[4 * i] != 0.f || mw[i] >= 0.f)) { printf("point %d: not finite, yet located\n", i); ++failures; }
        if (act[i]) {                                          // inside: the grid finds the same tet and weights
            ++inside;
            if (!(mw[i] >= 0.f) || tb[i] != ta[i] || memcmp(&ba[4 * i], &bb[4 * i], 16)) { printf("point %d: grid differs from exhaustive\n", i); ++failures; }
        } else if (mw[i] >= 0.f) { printf("point %d: the grid alone contains it\n", i); ++failures; }
    }
    if (inside < P / 4) { printf("only %d of %d points inside\n", inside, P); ++failures; }
    // 3-NN: the finite points, bucketed in cells of edge 0.3; then clouds of 0 .. 4 points
    const int Q = P - 3;
    float plo[3] = {INFINITY, INFINITY, INFINITY}, phi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int v = 0; v < 3 * Q; ++v) { plo[v % 3] = fminf(plo[v % 3], pts[v]); phi[v % 3] = fmaxf(phi[v % 3], pts[v]); }
    const float h = 0.3f, kor[4] = {plo[0], plo[1], plo[2], h};
    const int32_t kd[3] = {(int)ceilf((phi[0] - plo[0]) / h) + 1, (int)ceilf((phi[1] - plo[1]) / h) + 1, (int)ceilf((phi[2] - plo[2]) / h) + 1};
    std::vector<int> cell(3 * (size_t)Q);
    for (int v = 0; v < 3 * Q; ++v) cell[v] = clampi((int)floorf((pts[v] - plo[v % 3]) / h), kd[v % 3] - 1);
    csr(cell, cell, kd, start, items);
    std::vector<float> ka(Q), kb(Q);
    if (hc_knn3_mean_dist2(Q, pts.data(), ka.data()) || hc_knn3_mean_dist2_grid(Q, pts.data(), start.data(), items.data(), kor, kd, kb.data())) ++failures;
    if (memcmp(ka.data(), kb.data(), 4 * (size_t)Q)) { printf("3-NN: the ring search differs from the exhaustive one\n"); ++failures; }
    for (int n = 0; n <= 4; ++n) {
        std::vector<float> few(3 * (size_t)(n ? n : 1)), out(n ? n : 1, -7.f);
        for (auto &v : few) v = uniform();
        if (hc_knn3_mean_dist2(n, few.data(), out.data())) ++failures;
        if (n == 1 && out[0] != 0.f) { printf("3-NN of a single point is %g\n", out[0]); ++failures; }
    }
    printf(failures ? "locatecheck: %d failures\n" : "locatecheck: ok\n", failures);
    return failures != 0;
}
#endif
