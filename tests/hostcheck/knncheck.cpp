// knncheck.cpp -- csrc/knn_math.h (the K-nearest-neighbour arithmetic the kernels of knn.hip run) and mesh_interp_attr of
// csrc/mesh_raster_math.h on the CPU, built with g++ -ffp-contract=off as the device build is: the yardstick the GPU results are
// compared with bit for bit (tests/knn_ref.py loads it as a shared library).  With -DKNNCHECK_MAIN it is a stand-alone program
// that runs both searches on a small cloud -- queries outside the box, duplicates, K = 1 .. 16, P2 < K -- and compares them; that
// program is what gets built with -fsanitize=address,undefined.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../d3ga_amd/csrc/knn_math.h"
#include "../../d3ga_amd/csrc/mesh_raster_math.h"

using namespace d3ga;

template <int K>
static void exhaustive(int N, int P1, int P2, int k_out, const float *p1, const float *p2, float *dists, int64_t *idx) {
    for (int n = 0; n < N; ++n)
        for (int i = 0; i < P1; ++i) {
            const float *q = p1 + ((size_t)n * P1 + i) * 3;
            const float *cloud = p2 + (size_t)n * P2 * 3;
            float d[K];
            int32_t id[K];
            knn_clear<K>(d, id);
            for (int j = 0; j < P2; ++j) knn_consider<K>(d, id, cloud + 3 * (size_t)j, q[0], q[1], q[2], j);
            const size_t row = ((size_t)n * P1 + i) * (size_t)k_out;
            knn_store<K>(d, id, k_out, dists + row, idx + row);
        }
}

template <int K>
static void grid(int P1, int P2, int k_out, const float *p1, const float *p2, const int32_t *cell_start, const int32_t *cell_points,
                 const float *origin_h, const int32_t *dims, float *dists, int64_t *idx) {
    for (int i = 0; i < P1; ++i) {
        const float *q = p1 + (size_t)i * 3;
        float d[K];
        int32_t id[K];
        knn_clear<K>(d, id);
        knn_grid_search<K>(q[0], q[1], q[2], P2, p2, cell_start, cell_points, origin_h[0], origin_h[1], origin_h[2], origin_h[3], dims[0],
                           dims[1], dims[2], d, id);
        knn_store<K>(d, id, k_out, dists + (size_t)i * k_out, idx + (size_t)i * k_out);
    }
}

#define HC_DISPATCH(K, CALL)         \
    do {                             \
        if ((K) <= 1) { CALL(1); }   \
        else if ((K) <= 2) { CALL(2); } \
        else if ((K) <= 4) { CALL(4); } \
        else if ((K) <= 8) { CALL(8); } \
        else { CALL(16); }           \
    } while (0)

extern "C" int hc_knn_points(int N, int P1, int P2, int K, const float *p1, const float *p2, float *dists, int64_t *idx) {
    if (K < 1 || K > kKnnMaxK) return -2;
#define HC_CALL(KT) exhaustive<KT>(N, P1, P2, K, p1, p2, dists, idx)
    HC_DISPATCH(K, HC_CALL);
#undef HC_CALL
    return 0;
}

extern "C" int hc_knn_points_grid(int P1, int P2, int K, const float *p1, const float *p2, const int32_t *cell_start,
                                  const int32_t *cell_points, const float *origin_h, const int32_t *dims, float *dists, int64_t *idx) {
    if (K < 1 || K > kKnnMaxK) return -2;
#define HC_CALL(KT) grid<KT>(P1, P2, K, p1, p2, cell_start, cell_points, origin_h, dims, dists, idx)
    HC_DISPATCH(K, HC_CALL);
#undef HC_CALL
    return 0;
}

extern "C" int hc_interp_face_attrs(int64_t n_pix, int64_t F_total, int D, const int64_t *pix_to_face, const float *bary,
                                    const float *face_attrs, float *out) {
    for (int64_t p = 0; p < n_pix; ++p)
        for (int c = 0; c < D; ++c) {
            const int64_t f = pix_to_face[p];
            float v = 0.f;
            if (f >= 0 && f < F_total) {
                const float *a = face_attrs + (size_t)f * 3 * D + c;
                v = mesh_interp_attr(bary[3 * p], bary[3 * p + 1], bary[3 * p + 2], a[0], a[D], a[2 * D]);
            }
            out[p * D + c] = v;
        }
    return 0;
}

#ifdef KNNCHECK_MAIN
static uint32_t rng_state = 12345u;
static float uniform() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return (float)(rng_state >> 8) / 16777216.0f;
}

// the bucketing of d3ga_amd/knn.py (_grid): cells of edge h from the box's lower corner, ceil(span / h) + 1 cells per axis
static void bucket(const std::vector<float> &pts, float h, std::vector<int32_t> &start, std::vector<int32_t> &items, float *origin_h,
                   int32_t *dims) {
    const int P = (int)pts.size() / 3;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = 0; i < P; ++i)
        for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], pts[3 * i + a]); hi[a] = fmaxf(hi[a], pts[3 * i + a]); }
    for (int a = 0; a < 3; ++a) { origin_h[a] = lo[a]; dims[a] = (int)ceilf((hi[a] - lo[a]) / h) + 1; }
    origin_h[3] = h;
    const int cells = dims[0] * dims[1] * dims[2];
    std::vector<int> cell(P);
    start.assign(cells + 1, 0);
    for (int i = 0; i < P; ++i) {
        int c[3];
        for (int a = 0; a < 3; ++a) {
            c[a] = (int)floorf((pts[3 * i + a] - lo[a]) / h);
            c[a] = c[a] < 0 ? 0 : (c[a] > dims[a] - 1 ? dims[a] - 1 : c[a]);
        }
        cell[i] = (c[2] * dims[1] + c[1]) * dims[0] + c[0];
        ++start[cell[i] + 1];
    }
    for (int c = 0; c < cells; ++c) start[c + 1] += start[c];
    std::vector<int32_t> fill(start.begin(), start.end() - 1);
    items.assign(P > 0 ? P : 1, 0);
    for (int i = 0; i < P; ++i) items[fill[cell[i]]++] = i;
}

int main() {
    int failures = 0;
    const int sizes[][2] = {{257, 1000}, {64, 3}, {1, 500}, {300, 300}};
    for (const auto &sz : sizes) {
        const int P1 = sz[0], P2 = sz[1];
        std::vector<float> p2(3 * (size_t)P2), p1(3 * (size_t)P1);
        for (auto &v : p2) v = uniform();
        for (int i = P2 / 2; i < P2; i += 7)                   // duplicates: the tie rule
            memcpy(&p2[3 * (size_t)i], &p2[3 * (size_t)(i - P2 / 2)], 12);
        for (int i = 0; i < P1; ++i)
            for (int a = 0; a < 3; ++a) p1[3 * (size_t)i + a] = i % 3 == 0 ? 5.f * uniform() - 2.f : uniform();      // a third outside the box
        if (P1 == P2) p1 = p2;
        std::vector<int32_t> start, items;
        float origin_h[4];
        int32_t dims[3];
        bucket(p2, 0.17f, start, items, origin_h, dims);
        for (int K = 1; K <= kKnnMaxK; ++K) {
            std::vector<float> da((size_t)P1 * K), db((size_t)P1 * K);
            std::vector<int64_t> ia((size_t)P1 * K), ib((size_t)P1 * K);
            hc_knn_points(1, P1, P2, K, p1.data(), p2.data(), da.data(), ia.data());
            hc_knn_points_grid(P1, P2, K, p1.data(), p2.data(), start.data(), items.data(), origin_h, dims, db.data(), ib.data());
            if (memcmp(da.data(), db.data(), da.size() * 4) || memcmp(ia.data(), ib.data(), ia.size() * 8)) {
                printf("P1 %d P2 %d K %d: the grid search differs from the exhaustive one\n", P1, P2, K);
                ++failures;
            }
            for (size_t r = 0; r < (size_t)P1; ++r)
                for (int k = 1; k < K && k < P2; ++k)
                    if (da[r * K + k] < da[r * K + k - 1] || (da[r * K + k] == da[r * K + k - 1] && ia[r * K + k] <= ia[r * K + k - 1])) {
                        printf("P1 %d P2 %d K %d row %zu: not ascending in (distance, index)\n", P1, P2, K, r);
                        ++failures;
                    }
        }
    }
    // interpolation: background, an index past the end, D = 1 and 6
    for (int D : {1, 6}) {
        const int64_t n_pix = 37, F = 5;
        std::vector<int64_t> p2f(n_pix);
        std::vector<float> bary(3 * n_pix), attrs((size_t)F * 3 * D), out((size_t)n_pix * D, -7.f);
        for (int64_t p = 0; p < n_pix; ++p) p2f[p] = p % 7 - 1;       // -1 .. 5: background and one past the end
        for (auto &v : bary) v = uniform();
        for (auto &v : attrs) v = uniform();
        hc_interp_face_attrs(n_pix, F, D, p2f.data(), bary.data(), attrs.data(), out.data());
        for (int64_t p = 0; p < n_pix; ++p)
            if ((p2f[p] < 0 || p2f[p] >= F) && out[p * D] != 0.f) ++failures;
    }
    printf(failures ? "knncheck: %d failures\n" : "knncheck: ok\n", failures);
    return failures != 0;
}
#endif
