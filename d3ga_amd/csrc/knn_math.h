// knn_math.h -- the per-element arithmetic of the K-nearest-neighbour search (knn.hip): the squared distance, the (distance,
// index) order, the K-slot insertion, the bound of the grid search's stop rule and the padding of the result rows.
// Semantics: DESIGN.md 4.4j (specification of record; pytorch3d's knn_points as far as the reference's
// models/cage_net.py:66 can observe them).  Compiles for the host as it is (tests/hostcheck/knncheck.cpp runs this very text
// on the CPU against a float64 brute force); knn.hip is compiled with -ffp-contract=off, so the device evaluates every
// expression here as g++ does.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifndef D3GA_FHD
#ifdef __HIPCC__
#define D3GA_FHD __host__ __device__ __forceinline__
#else
#define D3GA_FHD static inline
#endif
#endif

namespace d3ga {

constexpr int kKnnMaxK = 16;                    // neighbours kept per query, at most
constexpr int32_t kKnnEmpty = 0x7fffffff;       // index of a slot nothing was inserted into (no point has it: P2 < 2^31 - 1)

// a - b rounded, and what the rounding lost (Knuth's two-sum: a - b == *d + *e exactly while nothing overflows).  The
// difference of two float32 coordinates is exact when they lie within a factor of two of each other and rounds otherwise --
// a query far outside the cloud -- and that rounding alone can cost 2 * 2^-24 of a squared distance.
D3GA_FHD void knn_diff(float a, float b, float *d, float *e) {
    const float c = -b, s = a + c;
    const float bp = s - a, ap = s - bp;
    *d = s;
    *e = (a - ap) + (c - bp);
}

// Squared Euclidean distance: dx*dx + dy*dy + dz*dz of the float32 differences, the expression of knn3_insert (bary.hip),
// three products and two additions left to right -- plus the first-order term 2 (dx ex + dy ey + dz ez) of what the three
// subtractions lost, so that the result stays within 4 * 2^-24 d of the distance of the float32 coordinates wherever the query
// lies (3 * 2^-24: the plain sum's 2.5 and the last addition's 0.5; the e^2 terms are below 2^-48 d).  Where the differences
// are exact the term is 0 and the value is the plain expression's, bit for bit.  Where the term is not a number (an infinite
// coordinate: inf - inf above) or would make the sum one, the plain sum stands.
D3GA_FHD float knn_dist2(const float *q, float px, float py, float pz) {
    float dx, dy, dz, ex, ey, ez;
    knn_diff(q[0], px, &dx, &ex);
    knn_diff(q[1], py, &dy, &ey);
    knn_diff(q[2], pz, &dz, &ez);
    const float plain = (dx * dx + dy * dy) + dz * dz;
    const float fixed = plain + 2.f * ((dx * ex + dy * ey) + dz * ez);
    return fixed == fixed ? fixed : plain;
}

// (distance, index) order: the lower index first on equal distances.  False whenever d is NaN.
D3GA_FHD bool knn_before(float d, int32_t j, float ds, int32_t js) { return d < ds || (d == ds && j < js); }

// The K slots hold the K smallest (distance, index) pairs seen so far, ascending; empty slots are (INFINITY, kKnnEmpty).
// Slot k becomes: the old slot k - 1 if the candidate goes before that one, the candidate if it goes before the old slot k
// only, else it stays.  No slot is indexed by a run-time value, so the arrays stay in registers.  The result is the same
// whatever the order of the candidates: pairs are distinct (indices are) and the order on them is total.
template <int K>
D3GA_FHD void knn_insert(float (&d)[K], int32_t (&id)[K], float c, int32_t j) {
    if (!knn_before(c, j, d[K - 1], id[K - 1])) return;       // not among the K best (or NaN)
#pragma unroll
    for (int k = K - 1; k > 0; --k) {
        const bool below = knn_before(c, j, d[k - 1], id[k - 1]);
        const bool here = knn_before(c, j, d[k], id[k]);
        d[k] = below ? d[k - 1] : (here ? c : d[k]);
        id[k] = below ? id[k - 1] : (here ? j : id[k]);
    }
    if (knn_before(c, j, d[0], id[0])) { d[0] = c; id[0] = j; }
}

// One candidate.  Most candidates are far beyond the K-th pair, and for them the plain sum decides at a third of the cost:
// |2 (dx ex + ...)| <= 2^-23 (1 + 2^-23) plain, since |ex| <= 2^-24 |dx|, so knn_dist2 >= plain (1 - 2^-22) > 0.99999 plain, and a
// candidate with 0.99999 plain > the K-th distance cannot be among the K best.  Everything else (NaN and infinity included, for
// which the comparison is false or undecided) goes through knn_dist2, so the slots hold the same pairs as without the shortcut.
template <int K>
D3GA_FHD void knn_consider(float (&d)[K], int32_t (&id)[K], const float *q, float px, float py, float pz, int32_t j) {
    const float dx = q[0] - px, dy = q[1] - py, dz = q[2] - pz;
    if (((dx * dx + dy * dy) + dz * dz) * 0.99999f > d[K - 1]) return;
    knn_insert<K>(d, id, knn_dist2(q, px, py, pz), j);
}

template <int K>
D3GA_FHD void knn_clear(float (&d)[K], int32_t (&id)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) { d[k] = INFINITY; id[k] = kKnnEmpty; }
}

// the first `k_out` slots -> one row of the result; pytorch3d pads the slots a cloud of fewer than K points leaves: 0, 0
template <int K>
D3GA_FHD void knn_store(const float (&d)[K], const int32_t (&id)[K], int k_out, float *dists, int64_t *idx) {
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (k < k_out) {
            const bool filled = id[k] != kKnnEmpty;
            dists[k] = filled ? d[k] : 0.f;
            idx[k] = filled ? (int64_t)id[k] : (int64_t)0;
        }
}

// ---- the grid search ---------------------------------------------------------------------------------------------------
// the cell of a coordinate, clamped into the grid (a query outside the box starts from the nearest boundary cell; NaN -> 0)
D3GA_FHD int knn_cell(float x, float o, float inv_h, int n) {
    const float c = fminf(fmaxf(floorf((x - o) * inv_h), 0.f), (float)(n - 1));
    return (int)c;
}

// One axis of the stop rule.  The cells [c - r, c + r] of this axis have been visited (clipped to [0, n - 1]); a point not yet
// seen that differs from the block along this axis lies in a cell < c - r or > c + r, i.e. beyond the plane  o + (c - r) h  or
// o + (c + r + 1) h.  -> the query's TRUE distance to the nearer of the two planes that still have cells behind them
// (INFINITY if neither has), never below 0, shortened by `slack`: the caller's bucketing and these planes are both rounded in
// float32, and a bound that is too small only costs another ring.
D3GA_FHD float knn_axis_reach(float x, float o, float h, int c, int r, int n) {
    float reach = INFINITY;
    if (c - r > 0) {
        const float plane = o + (float)(c - r) * h;
        const float slack = 9.5367431640625e-7f * ((fabsf(plane) + fabsf(o)) + fabsf(x));      // 2^-20
        reach = fminf(reach, (x - plane) - slack);
    }
    if (c + r < n - 1) {
        const float plane = o + (float)(c + r + 1) * h;
        const float slack = 9.5367431640625e-7f * ((fabsf(plane) + fabsf(o)) + fabsf(x));
        reach = fminf(reach, (plane - x) - slack);
    }
    return fmaxf(reach, 0.f);                                  // NaN -> 0: never stops early
}

// The ring search of one query over p2 bucketed in a uniform grid (CSR cell_start / cell_points).  Rings r = 0, 1, ... of cells
// at Chebyshev distance r from the query's clamped cell; it stops once the K-th pair lies STRICTLY inside the reach of the
// visited block (an unseen pair at the very same distance could still win the tie on its index).  Every loop is bounded by
// the grid dimensions; a CSR entry outside [0, P2) is skipped, so nothing outside p2 is read.
template <int K>
D3GA_FHD void knn_grid_search(float px, float py, float pz, int P2, const float *p2, const int32_t *cell_start,
                              const int32_t *cell_points, float ox, float oy, float oz, float h, int nx, int ny, int nz,
                              float (&d)[K], int32_t (&id)[K]) {
    const float inv_h = 1.0f / h;
    const int cx = knn_cell(px, ox, inv_h, nx), cy = knn_cell(py, oy, inv_h, ny), cz = knn_cell(pz, oz, inv_h, nz);
    const int rmax = nx > ny ? (nx > nz ? nx : nz) : (ny > nz ? ny : nz);      // ring rmax - 1 reaches every cell from any cell
    for (int r = 0; r < rmax; ++r) {
        if (r > 0) {
            const float reach = fminf(fminf(knn_axis_reach(px, ox, h, cx, r - 1, nx), knn_axis_reach(py, oy, h, cy, r - 1, ny)),
                                      knn_axis_reach(pz, oz, h, cz, r - 1, nz));
            if (d[K - 1] < reach * reach) break;
        }
        const int z0 = cz - r > 0 ? cz - r : 0, z1 = cz + r < nz - 1 ? cz + r : nz - 1;
        const int y0 = cy - r > 0 ? cy - r : 0, y1 = cy + r < ny - 1 ? cy + r : ny - 1;
        const int x0 = cx - r > 0 ? cx - r : 0, x1 = cx + r < nx - 1 ? cx + r : nx - 1;
        for (int z = z0; z <= z1; ++z)
            for (int y = y0; y <= y1; ++y) {
                // a row of the shell is whole on the shell's faces, else only its two end cells are on the shell
                const bool whole = r == 0 || z == cz - r || z == cz + r || y == cy - r || y == cy + r;
                const int step = whole ? 1 : 2 * r;
                for (int x = whole ? x0 : cx - r; x <= x1; x += step) {
                    if (x < x0) continue;
                    const int cell = (z * ny + y) * nx + x;
                    int begin = cell_start[cell], end = cell_start[cell + 1];
                    if (begin < 0) begin = 0;
                    if (end > P2) end = P2;
                    for (int k = begin; k < end; ++k) {
                        const int32_t j = cell_points[k];
                        if ((uint32_t)j < (uint32_t)P2) knn_consider<K>(d, id, p2 + 3 * (size_t)j, px, py, pz, j);
                    }
                }
            }
    }
}

}  // namespace d3ga
