// bary_math.h -- the per-element arithmetic of the init-time point location and 3-NN scale seed (bary.hip): the scalar triple
// product, the barycentric weights of a point in a tetrahedron and their minimum, the two selection rules (exhaustive: strict
// >, the tets arrive in ascending index; grid: >, or equal and the lower index), the three-slot insertion and the mean.
// Weights follow submodules/tetrahedralize/include/tet/tetrahedron.h:77-101 (order a,b,c,d = corners 0..3).
// Compiles for the host as it is (tests/hostcheck/locatecheck.cpp runs this very text on the CPU against a float64 oracle);
// bary.hip is compiled with -ffp-contract=off and correctly rounded division, so the device evaluates every expression here
// as g++ does.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "d3ga_math.h"
#include "knn_math.h"

#ifndef D3GA_FHD
#ifdef __HIPCC__
#define D3GA_FHD __host__ __device__ __forceinline__
#else
#define D3GA_FHD static inline
#endif
#endif

namespace d3ga {

constexpr int32_t kBaryNoTet = 0x7fffffff;     // best index of the grid search before any candidate was taken

D3GA_FHD float stp(V3 a, V3 b, V3 c) {   // a . (b x c)
    return a.x * (b.y * c.z - b.z * c.y) + a.y * (b.z * c.x - b.x * c.z) + a.z * (b.x * c.y - b.y * c.x);
}

// weights of p in the tet (a,b,c,d) and their minimum -- ONE definition for the exhaustive and the grid kernel, so that both
// produce bit-identical numbers for the same (point, tet).  A tet whose six-fold volume evaluates to 0, or whose weights are
// not all finite (1 / 0 and overflow turn rounding noise into weights; a NaN or infinite point), has minimum -INFINITY: the
// strict > of both selection rules never takes it.  Slivers of tiny non-zero volume are ordinary tets.
struct TetW { float w[4]; float mn; };
D3GA_FHD TetW tet_weights(V3 p, const float *c) {
    const V3 a = v3(c[0], c[1], c[2]), b = v3(c[3], c[4], c[5]), cc = v3(c[6], c[7], c[8]), d = v3(c[9], c[10], c[11]);
    const V3 vap = p - a, vbp = p - b, vab = b - a, vac = cc - a, vad = d - a, vbc = cc - b, vbd = d - b;
    const float vol6 = stp(vab, vac, vad);
    const float v6 = 1.0f / vol6;
    TetW r;
    r.w[0] = stp(vbp, vbd, vbc) * v6; r.w[1] = stp(vap, vac, vad) * v6; r.w[2] = stp(vap, vad, vab) * v6;
    r.w[3] = stp(vap, vab, vac) * v6;
    r.mn = fminf(fminf(r.w[0], r.w[1]), fminf(r.w[2], r.w[3]));
    const bool finite = fabsf(r.w[0]) < INFINITY && fabsf(r.w[1]) < INFINITY && fabsf(r.w[2]) < INFINITY && fabsf(r.w[3]) < INFINITY;
    if (vol6 == 0.f || !finite) r.mn = -INFINITY;
    return r;
}

// the running best of a search: weights, tet, minimum weight
struct BaryBest { float w[4]; float mn; int32_t t; };
D3GA_FHD void bary_best_clear(BaryBest &b, int32_t t0) {
    b.w[0] = 0.f; b.w[1] = 0.f; b.w[2] = 0.f; b.w[3] = 0.f;
    b.mn = -INFINITY; b.t = t0;
}
D3GA_FHD void bary_best_take(BaryBest &b, const TetW &tw, int32_t t) {
    b.mn = tw.mn; b.t = t;
    b.w[0] = tw.w[0]; b.w[1] = tw.w[1]; b.w[2] = tw.w[2]; b.w[3] = tw.w[3];
}
// exhaustive search, tets visited in ascending index
D3GA_FHD void bary_select_exhaustive(BaryBest &b, const TetW &tw, int32_t t) {
    if (tw.mn > b.mn) bary_best_take(b, tw, t);         // strict: ties keep the lowest tet index
}
// grid search, candidates in the order of the cell's list
D3GA_FHD void bary_select_grid(BaryBest &b, const TetW &tw, int32_t t) {
    if (!(tw.mn > -INFINITY)) return;                   // a degenerate tet is never taken (-INFINITY == the cleared minimum)
    if (tw.mn > b.mn || (tw.mn == b.mn && t < b.t)) bary_best_take(b, tw, t);
}
// one chunk of the exhaustive search: cnt tets (12 floats each, from LDS on the device) whose first has index base
constexpr int kBaryChunk = 256;
D3GA_FHD void bary_scan_chunk(BaryBest &b, V3 p, const float *chunk, int base, int cnt) {
    for (int j = 0; j < cnt; ++j) bary_select_exhaustive(b, tet_weights(p, chunk + 12 * j), base + j);
}
// the grid cell of a coordinate (before the range test)
D3GA_FHD int bary_cell(float x, float o, float inv_h) {
    const float f = floorf((x - o) * inv_h);
    return f >= -1.f && f < 2147483648.f ? (int)f : -1;    // NaN and what no int holds: outside every grid
}
D3GA_FHD int bary_imin(int a, int b) { return a < b ? a : b; }
D3GA_FHD int bary_imax(int a, int b) { return a > b ? a : b; }

// keeps the three smallest squared distances (ascending) -- shared by the exhaustive and the grid kernel.  The distance is
// knn_dist2 (knn_math.h), the one knn_points returns: dx*dx + dy*dy + dz*dz of the float32 differences q - p, made up for what
// the three subtractions lost (nothing where they are exact: the plain expression's value, bit for bit).  With the plain
// expression the mean differed from knn_points(p, p, K=4)'s by up to 3 ulps on a uniform cloud.
D3GA_FHD void knn3_insert(V3 p, const float *q, float &d0, float &d1, float &d2) {
    const float d = knn_dist2(q, p.x, p.y, p.z);
    if (d < d2) {
        if (d < d1) {
            d2 = d1;
            if (d < d0) { d1 = d0; d0 = d; } else { d1 = d; }
        } else {
            d2 = d;
        }
    }
}
// knn_points(p, p, K=4)[0][0, :, 1:].mean(-1) (models/cage_net.py:66): a mean over THREE slots; with fewer than three other
// points pytorch3d pads the missing distances with 0, so the sum of what exists is divided by 3 as well
D3GA_FHD float knn3_mean(float d0, float d1, float d2) {
    float sum = 0.f;
    if (d0 < INFINITY) sum += d0;
    if (d1 < INFINITY) sum += d1;
    if (d2 < INFINITY) sum += d2;
    return sum / 3.0f;
}

// The ring search of the grid kernel for one point i of the cloud (CSR cell_start / cell_points over cells of edge h): cells
// at Chebyshev ring r = 0, 1, 2, ... around the point's own; stops as soon as the third-smallest distance is within (r-1) h.
D3GA_FHD float knn3_grid_search(int i, const float *points, const int32_t *cell_start, const int32_t *cell_points, float ox, float oy,
                                float oz, float h, int nx, int ny, int nz) {
    const V3 p = v3(points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2]);
    const float inv_h = 1.0f / h;
    const int cx = bary_imin(bary_imax((int)floorf((p.x - ox) * inv_h), 0), nx - 1), cy = bary_imin(bary_imax((int)floorf((p.y - oy) * inv_h), 0), ny - 1);
    const int cz = bary_imin(bary_imax((int)floorf((p.z - oz) * inv_h), 0), nz - 1);
    float d0 = INFINITY, d1 = INFINITY, d2 = INFINITY;
    const int rmax = bary_imax(nx, bary_imax(ny, nz));
    for (int r = 0; r <= rmax; ++r) {
        if (r > 0) {
            const float reach = (float)(r - 1) * h;                    // everything within ring r-1 has been seen
            if (d2 <= reach * reach) break;
        }
        auto visit = [&](int x, int y, int z) {
            const int cell = (z * ny + y) * nx + x;
            for (int k = cell_start[cell]; k < cell_start[cell + 1]; ++k) {
                const int j = cell_points[k];
                if (j != i) knn3_insert(p, points + 3 * (size_t)j, d0, d1, d2);
            }
        };
        for (int z = bary_imax(cz - r, 0); z <= bary_imin(cz + r, nz - 1); ++z)
            for (int y = bary_imax(cy - r, 0); y <= bary_imin(cy + r, ny - 1); ++y) {
                const bool face = (z == cz - r) || (z == cz + r) || (y == cy - r) || (y == cy + r);
                if (face || r == 0) {                                  // a whole row of the shell
                    for (int x = bary_imax(cx - r, 0); x <= bary_imin(cx + r, nx - 1); ++x) visit(x, y, z);
                } else {                                               // interior row: only its two end cells are on the shell
                    if (cx - r >= 0) visit(cx - r, y, z);
                    if (cx + r < nx) visit(cx + r, y, z);
                }
            }
    }
    return knn3_mean(d0, d1, d2);
}

}  // namespace d3ga
