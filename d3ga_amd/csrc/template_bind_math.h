// template_bind_math.h -- the rules of template binding (template_bind.hip): one level of Loop subdivision that
// carries attribute columns along (the reference's utils/mesh_utils.py::subdivide_loop :105-325) and the closed form of
// lib/smplman.py::Smplman.unpose :55-59.  Compiles for the host as it is: tests/hostcheck/template_bind_host.cpp runs this very text on
// the CPU against tests/template_bind_ref.py; template_bind.hip is compiled with -ffp-contract=off, so the device evaluates every
// expression here as g++ does (fp64 division is correctly rounded on both).  No library call: beta_k comes from a table.
//
// All arithmetic is float64 with ONE rounding to float32 per output element.  Every sum has a fixed order:
//   keys     face edge h = 3 f + c joins (faces[f][c], faces[f][(c + 1) % 3]); key = larger << 32 | smaller.  A face that names a
//            vertex outside [0, V) (STATUS_RANGE) or one vertex twice (STATUS_DEGENERATE) has the key D3GA_LOOP_BAD_KEY: it sorts last
//            and takes no part.  The keys are sorted ascending and STABLY, so a run of equal keys lists its face edges ascending.
//   edges    a run of equal keys is one unique edge; edges are numbered in run order, which is ascending (larger, smaller).  The
//            first member of the run is the face of lower index, the second the other face; a third sets STATUS_NONMANIFOLD and is
//            left out.  The opposite vertex of face edge (f, c) is faces[f][(c + 2) % 3].  A run of one is a boundary edge.
//   vertices valence = number of unique edges at the vertex; a boundary vertex is an end of a boundary edge; neighbours ascending.
//   odd      interior:  ((0.375 x0 + 0.375 x1) + x2 / 8) + x3 / 8   x0 the smaller endpoint, x2 opposite in the face of lower index
//            boundary:  (x0 + x1) 0.5
//   even     interior:  beta[k] S + (1 - k beta[k]) x, S = ((0 + x_n0) + x_n1) + ... over the neighbours in ascending index order
//            boundary:  S' / 8 + 0.75 x, S' the same sum over the neighbours that are boundary vertices -- every one of them, also
//                       across an interior edge (the reference's rule; on the two-triangle quad the weights sum to 9/8)
//            a vertex of no face keeps x.
//   unpose   [M t; 0 0 0 s] = sum over the row's (joint, weight) pairs in stored order, pairs of weight 0 skipped, each entry
//            acc += w A[j][e] starting from 0; s = the sum of the weights, the same way.  d = v - t / s;
//            det = (m00 (m11 m22 - m12 m21) - m01 (m10 m22 - m12 m20)) + m02 (m10 m21 - m11 m20);
//            x_i = ((c_i0 d0 + c_i1 d1) + c_i2 d2) / det - offset_i, c the transposed cofactors.  |det| < kTbMinDet or
//            |s| < kTbMinScale (or either not a number): STATUS_SINGULAR and a row of zeros, never NaN or Inf from a singular blend.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/d3ga.h"

#ifndef D3GA_FHD
#ifdef __HIPCC__
#define D3GA_FHD __host__ __device__ __forceinline__
#else
#define D3GA_FHD static inline
#endif
#endif

namespace d3ga {

constexpr int kTbBlock = 256;                                // items per first-level scan block (= the workgroup)
constexpr double kTbMinDet = 1e-12;                          // |det M| below this: the blend is singular (rotations blend to det <= 1)
constexpr double kTbMinScale = 1e-12;                        // |sum of weights| below this: no blend to invert
constexpr int64_t kTbBadKey = D3GA_LOOP_BAD_KEY;

// ---- keys ---------------------------------------------------------------------------------------------------------------------------
D3GA_FHD int64_t tb_edge_key(int32_t V, const int32_t *faces, int64_t h, uint32_t *flags) {
    const int32_t *t = faces + 3 * (h / 3);
    if ((uint32_t)t[0] >= (uint32_t)V || (uint32_t)t[1] >= (uint32_t)V || (uint32_t)t[2] >= (uint32_t)V) {
        *flags |= D3GA_BIND_STATUS_RANGE;
        return kTbBadKey;
    }
    if (t[0] == t[1] || t[1] == t[2] || t[2] == t[0]) {
        *flags |= D3GA_BIND_STATUS_DEGENERATE;
        return kTbBadKey;
    }
    const int c = (int)(h % 3);
    const int32_t a = t[c], b = t[(c + 1) % 3];
    const int32_t lo = a < b ? a : b, hi = a < b ? b : a;
    return ((int64_t)hi << 32) | (int64_t)lo;
}

// ---- edges --------------------------------------------------------------------------------------------------------------------------
D3GA_FHD int32_t tb_is_head(const int64_t *keys, int64_t p) { return keys[p] != kTbBadKey && (p == 0 || keys[p] != keys[p - 1]) ? 1 : 0; }

struct TbEdge {
    int32_t lo, hi, f0, f1, o0, o1;
    bool boundary;
};

// the unique edge whose run starts at sorted position p (tb_is_head(keys, p)); n = 3 F
D3GA_FHD TbEdge tb_edge_at(int32_t V, int64_t n, const int64_t *keys, const int64_t *perm, const int32_t *faces, int64_t p, uint32_t *flags) {
    const int64_t key = keys[p];
    TbEdge e;
    e.lo = (int32_t)(key & 0xffffffffLL);
    e.hi = (int32_t)(key >> 32);
    const int count = 1 + (p + 1 < n && keys[p + 1] == key ? 1 : 0) + (p + 2 < n && keys[p + 1] == key && keys[p + 2] == key ? 1 : 0);
    if (count >= 3) *flags |= D3GA_BIND_STATUS_NONMANIFOLD;
    e.boundary = count == 1;
    int64_t h0 = perm[p], h1 = count >= 2 ? perm[p + 1] : -1;
    if ((uint64_t)h0 >= (uint64_t)n) { *flags |= D3GA_BIND_STATUS_RANGE; h0 = -1; }
    if (count >= 2 && (uint64_t)h1 >= (uint64_t)n) { *flags |= D3GA_BIND_STATUS_RANGE; h1 = -1; e.boundary = true; }
    e.f0 = h0 < 0 ? -1 : (int32_t)(h0 / 3);
    e.f1 = h1 < 0 ? -1 : (int32_t)(h1 / 3);
    e.o0 = h0 < 0 ? -1 : faces[3 * (h0 / 3) + (h0 % 3 + 2) % 3];
    e.o1 = h1 < 0 ? -1 : faces[3 * (h1 / 3) + (h1 % 3 + 2) % 3];
    if ((uint32_t)e.lo >= (uint32_t)V || (uint32_t)e.hi >= (uint32_t)V) { *flags |= D3GA_BIND_STATUS_RANGE; e.lo = e.hi = -1; }
    return e;
}

// One vertex's neighbours, ascending, in place (they are distinct -- one per unique edge -- so the result does not depend on the
// order they arrived in): insertion up to kTbInsertionMax entries, a heap sort beyond, so that one lane's work stays
// O(k log k) on a fan of any valence.
constexpr int32_t kTbInsertionMax = 16;
D3GA_FHD void tb_sift_down(int32_t *a, int32_t root, int32_t n) {
    for (;;) {
        int32_t child = 2 * root + 1;
        if (child >= n) return;
        if (child + 1 < n && a[child + 1] > a[child]) ++child;
        if (a[root] >= a[child]) return;
        const int32_t t = a[root];
        a[root] = a[child];
        a[child] = t;
        root = child;
    }
}
D3GA_FHD void tb_sort_segment(int32_t *nbr, int32_t begin, int32_t end) {
    int32_t *a = nbr + begin;
    const int32_t n = end - begin;
    if (n <= kTbInsertionMax) {
        for (int32_t i = 1; i < n; ++i) {
            const int32_t x = a[i];
            int32_t j = i - 1;
            while (j >= 0 && a[j] > x) { a[j + 1] = a[j]; --j; }
            a[j + 1] = x;
        }
        return;
    }
    for (int32_t i = n / 2 - 1; i >= 0; --i) tb_sift_down(a, i, n);
    for (int32_t m = n - 1; m > 0; --m) {
        const int32_t t = a[0];
        a[0] = a[m];
        a[m] = t;
        tb_sift_down(a, 0, m);
    }
}

// ---- stencils -------------------------------------------------------------------------------------------------------------------------
D3GA_FHD double tb_at(const double *x, int32_t D, int32_t row, int32_t col) { return x[(size_t)row * (size_t)D + (size_t)col]; }
D3GA_FHD bool tb_vertex_ok(const d3ga_loop_plan &p, int32_t v) { return (uint32_t)v < (uint32_t)p.V; }

D3GA_FHD double tb_odd(const d3ga_loop_plan &p, const double *x, int32_t D, int32_t col, int32_t e, uint32_t *flags) {
    const int32_t v0 = p.edge_verts[2 * (size_t)e], v1 = p.edge_verts[2 * (size_t)e + 1];
    if (!tb_vertex_ok(p, v0) || !tb_vertex_ok(p, v1)) { *flags |= D3GA_BIND_STATUS_RANGE; return 0.0; }
    const double x0 = tb_at(x, D, v0, col), x1 = tb_at(x, D, v1, col);
    if (p.edge_boundary[e]) return (x0 + x1) * 0.5;
    const int32_t v2 = p.edge_opp[2 * (size_t)e], v3 = p.edge_opp[2 * (size_t)e + 1];
    if (!tb_vertex_ok(p, v2) || !tb_vertex_ok(p, v3)) { *flags |= D3GA_BIND_STATUS_RANGE; return 0.0; }
    return ((0.375 * x0 + 0.375 * x1) + tb_at(x, D, v2, col) / 8.0) + tb_at(x, D, v3, col) / 8.0;
}

D3GA_FHD double tb_even(const d3ga_loop_plan &p, const double *x, int32_t D, int32_t col, int32_t v, const double *beta, int32_t n_beta,
                        uint32_t *flags) {
    const double xv = tb_at(x, D, v, col);
    const int32_t begin = p.vert_offsets[v], end = p.vert_offsets[v + 1];
    const int64_t k = (int64_t)end - begin;
    if (k <= 0) return xv;                                   // no face names the vertex: kept
    if (begin < 0 || (int64_t)end > 2 * (int64_t)p.E || k >= n_beta) { *flags |= D3GA_BIND_STATUS_RANGE; return xv; }
    const bool boundary = p.vert_boundary[v] != 0;
    double sum = 0.0;
    for (int32_t j = begin; j < end; ++j) {
        const int32_t nb = p.vert_nbr[j];
        if (!tb_vertex_ok(p, nb)) { *flags |= D3GA_BIND_STATUS_RANGE; continue; }
        if (boundary && !p.vert_boundary[nb]) continue;
        sum += tb_at(x, D, nb, col);
    }
    if (boundary) return sum / 8.0 + 0.75 * xv;
    const double b = beta[k];
    return b * sum + (1.0 - (double)k * b) * xv;
}

// element i of the (V + E, D) output
D3GA_FHD float tb_stencil(const d3ga_loop_plan &p, const double *x, int32_t D, int64_t i, const double *beta, int32_t n_beta, uint32_t *flags) {
    const int64_t row = i / D;
    const int32_t col = (int32_t)(i % D);
    return (float)(row < p.V ? tb_even(p, x, D, col, (int32_t)row, beta, n_beta, flags) : tb_odd(p, x, D, col, (int32_t)(row - p.V), flags));
}

// the four faces of face f: 12 indices
D3GA_FHD void tb_face_rows(const d3ga_loop_plan &p, const int32_t *faces, int32_t f, int32_t *out) {
    const int32_t a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
    const int32_t e0 = p.face_edge[3 * (size_t)f], e1 = p.face_edge[3 * (size_t)f + 1], e2 = p.face_edge[3 * (size_t)f + 2];
    const int32_t o0 = e0 < 0 ? -1 : p.V + e0, o1 = e1 < 0 ? -1 : p.V + e1, o2 = e2 < 0 ? -1 : p.V + e2;
    const int32_t rows[12] = {a, o0, o2, o0, b, o1, o2, o1, c, o0, o1, o2};
    for (int i = 0; i < 12; ++i) out[i] = rows[i];
}

// ---- unpose ---------------------------------------------------------------------------------------------------------------------------
struct TbUnpose {
    int32_t n, J, R, K, n_offsets;
    const double *vertices, *joint_mats, *offsets;
    const int32_t *skin_idx;                                 // NULL: the dense table, K = J
    const int64_t *rows;                                     // NULL: row i
};

template <typename TW>
D3GA_FHD void tb_unpose_one(const TbUnpose &u, const TW *skin_w, int32_t i, float *out, uint32_t *flags) {
    out[0] = out[1] = out[2] = 0.f;
    const int64_t r = u.rows ? u.rows[i] : (int64_t)i;
    if (r < 0 || r >= u.R || (u.offsets && r >= u.n_offsets)) { *flags |= D3GA_BIND_STATUS_RANGE; return; }
    double T[12] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, s = 0.0;
    for (int32_t k = 0; k < u.K; ++k) {
        const double w = (double)skin_w[(size_t)r * (size_t)u.K + (size_t)k];
        if (w == 0.0) continue;
        const int32_t j = u.skin_idx ? u.skin_idx[(size_t)r * (size_t)u.K + (size_t)k] : k;
        if ((uint32_t)j >= (uint32_t)u.J) { *flags |= D3GA_BIND_STATUS_RANGE; continue; }
        const double *A = u.joint_mats + 16 * (size_t)j;
        for (int e = 0; e < 12; ++e) T[e] += w * A[e];
        s += w;
    }
    const double m00 = T[0], m01 = T[1], m02 = T[2], m10 = T[4], m11 = T[5], m12 = T[6], m20 = T[8], m21 = T[9], m22 = T[10];
    const double det = (m00 * (m11 * m22 - m12 * m21) - m01 * (m10 * m22 - m12 * m20)) + m02 * (m10 * m21 - m11 * m20);
    if (!(fabs(det) >= kTbMinDet) || !(fabs(s) >= kTbMinScale) || !(fabs(det) <= 1.7976931348623157e308) || !(fabs(s) <= 1.7976931348623157e308)) {
        *flags |= D3GA_BIND_STATUS_SINGULAR;
        return;
    }
    const double *v = u.vertices + 3 * (size_t)i;
    const double d0 = v[0] - T[3] / s, d1 = v[1] - T[7] / s, d2 = v[2] - T[11] / s;
    const double c00 = m11 * m22 - m12 * m21, c01 = m02 * m21 - m01 * m22, c02 = m01 * m12 - m02 * m11;
    const double c10 = m12 * m20 - m10 * m22, c11 = m00 * m22 - m02 * m20, c12 = m02 * m10 - m00 * m12;
    const double c20 = m10 * m21 - m11 * m20, c21 = m01 * m20 - m00 * m21, c22 = m00 * m11 - m01 * m10;
    double x0 = ((c00 * d0 + c01 * d1) + c02 * d2) / det, x1 = ((c10 * d0 + c11 * d1) + c12 * d2) / det, x2 = ((c20 * d0 + c21 * d1) + c22 * d2) / det;
    if (u.offsets) {
        const double *b = u.offsets + 3 * (size_t)r;
        x0 -= b[0]; x1 -= b[1]; x2 -= b[2];
    }
    if (!(fabs(x0) <= 3.4028234663852886e38) || !(fabs(x1) <= 3.4028234663852886e38) || !(fabs(x2) <= 3.4028234663852886e38)) {
        *flags |= D3GA_BIND_STATUS_SINGULAR;                 // beyond float32 (or an input that is not a number): zeros, flagged
        return;
    }
    out[0] = (float)x0; out[1] = (float)x1; out[2] = (float)x2;
}

// ---- scratch layout and the argument rules of the entry points (include/d3ga.h); nothing is dereferenced ----------------------------------
//   [0] head     3 F int32      1 where a run of equal keys starts
//   [1] excl     3 F + 1 int32  exclusive prefix of head; excl[3 F] = E
//   [2] valence  V int32        (zeroed by the build)
//   [3] cursor   V int32        (zeroed by the build)
//   [4] block_total  nblk uint32     nblk = blocks of kTbBlock items over max(3 F, V)
//   [5] block_start  nblk + 1 uint64
static inline int64_t tb_align256(int64_t x) { return (x + 255) & ~int64_t(255); }
static inline int64_t tb_blocks(int64_t n) { return (n + kTbBlock - 1) / kTbBlock; }
static inline int64_t tb_scan_blocks(int64_t V, int64_t F) { return tb_blocks(3 * F > V ? 3 * F : V); }
static inline int64_t tb_scratch_bytes(int64_t V, int64_t F) {
    return tb_align256(12 * F) + tb_align256(4 * (3 * F + 1)) + 2 * tb_align256(4 * V) + tb_align256(4 * tb_scan_blocks(V, F)) +
           tb_align256(8 * (tb_scan_blocks(V, F) + 1));
}

struct TbScratch {
    int32_t *head, *excl, *valence, *cursor;
    uint32_t *block_total;
    uint64_t *block_start;
};
static inline TbScratch tb_carve(void *base, int64_t V, int64_t F) {
    char *p = static_cast<char *>(base);
    TbScratch s;
    s.head = reinterpret_cast<int32_t *>(p);          p += tb_align256(12 * F);
    s.excl = reinterpret_cast<int32_t *>(p);          p += tb_align256(4 * (3 * F + 1));
    s.valence = reinterpret_cast<int32_t *>(p);       p += tb_align256(4 * V);
    s.cursor = reinterpret_cast<int32_t *>(p);        p += tb_align256(4 * V);
    s.block_total = reinterpret_cast<uint32_t *>(p);  p += tb_align256(4 * tb_scan_blocks(V, F));
    s.block_start = reinterpret_cast<uint64_t *>(p);
    return s;
}

static inline int tb_check_sizes(int32_t V, int32_t F) {
    if (V <= 0 || F <= 0 || 6 * (int64_t)F > (int64_t)INT32_MAX) return D3GA_E_SIZE;     // 2 E <= 6 F entries of neighbour lists
    return 0;
}
static inline bool tb_odd_address(const void *p, uintptr_t mask) { return ((uintptr_t)p & mask) != 0; }

static inline int tb_check_keys(int32_t V, int32_t F, const int32_t *faces, const int64_t *keys, const uint32_t *status) {
    if (tb_check_sizes(V, F) != 0) return D3GA_E_SIZE;
    if (!faces || !keys || !status) return D3GA_E_NULL;
    if (tb_odd_address(faces, 3) || tb_odd_address(keys, 7) || tb_odd_address(status, 3)) return D3GA_E_CONFIG;
    return 0;
}

static inline int tb_check_plan(const d3ga_loop_plan *p, bool built) {
    if (!p) return D3GA_E_NULL;
    if (tb_check_sizes(p->V, p->F) != 0) return D3GA_E_SIZE;
    if (built && (p->E <= 0 || p->E > 3 * (int64_t)p->F || (int64_t)p->V + p->E > INT32_MAX)) return D3GA_E_SIZE;
    if (!p->edge_verts || !p->edge_opp || !p->edge_faces || !p->edge_boundary || !p->face_edge || !p->vert_offsets || !p->vert_nbr ||
        !p->vert_boundary) return D3GA_E_NULL;
    if (tb_odd_address(p->edge_verts, 3) || tb_odd_address(p->edge_opp, 3) || tb_odd_address(p->edge_faces, 3) || tb_odd_address(p->face_edge, 3) ||
        tb_odd_address(p->vert_offsets, 3) || tb_odd_address(p->vert_nbr, 3)) return D3GA_E_CONFIG;
    return 0;
}

static inline int tb_check_build(const d3ga_loop_plan *p, const int32_t *faces, const int64_t *keys, const int64_t *perm, const int32_t *info,
                                 const void *scratch, int64_t scratch_bytes) {
    const int st = tb_check_plan(p, false);
    if (st != 0) return st;
    if (!faces || !keys || !perm || !info || !scratch) return D3GA_E_NULL;
    if (tb_odd_address(faces, 3) || tb_odd_address(keys, 7) || tb_odd_address(perm, 7) || tb_odd_address(info, 3) || tb_odd_address(scratch, 255))
        return D3GA_E_CONFIG;
    if (scratch_bytes < tb_scratch_bytes(p->V, p->F)) return D3GA_E_CAPACITY;
    return 0;
}

static inline int tb_check_subdivide(const d3ga_loop_plan *p, int32_t D, const double *x, const double *beta, int32_t n_beta, const float *out,
                                     const uint32_t *status) {
    if (p && (D <= 0 || n_beta <= 0)) return D3GA_E_SIZE;
    const int st = tb_check_plan(p, true);
    if (st != 0) return st;
    if (!x || !beta || !out || !status) return D3GA_E_NULL;
    if (tb_odd_address(x, 7) || tb_odd_address(beta, 7) || tb_odd_address(out, 3) || tb_odd_address(status, 3)) return D3GA_E_CONFIG;
    return 0;
}

static inline int tb_check_faces(const d3ga_loop_plan *p, const int32_t *faces, const int32_t *out) {
    const int st = tb_check_plan(p, true);
    if (st != 0) return st;
    if (!faces || !out) return D3GA_E_NULL;
    if (tb_odd_address(faces, 3) || tb_odd_address(out, 3)) return D3GA_E_CONFIG;
    return 0;
}

static inline int tb_check_unpose(int32_t n, int32_t J, int32_t R, int32_t K, const double *vertices, const double *joint_mats, const void *skin_w,
                                  int32_t w_f64, const int32_t *skin_idx, const int64_t *rows, const double *offsets, int32_t n_offsets,
                                  const float *out, const uint32_t *status) {
    if (n <= 0 || J <= 0 || R <= 0 || K <= 0 || (int64_t)R * K > INT32_MAX || 16 * (int64_t)J > INT32_MAX || 3 * (int64_t)n > INT32_MAX)
        return D3GA_E_SIZE;
    if (!skin_idx && K != J) return D3GA_E_SIZE;
    if (offsets && n_offsets <= 0) return D3GA_E_SIZE;
    if (!vertices || !joint_mats || !skin_w || !out || !status) return D3GA_E_NULL;
    if (w_f64 != 0 && w_f64 != 1) return D3GA_E_CONFIG;
    if (tb_odd_address(vertices, 7) || tb_odd_address(joint_mats, 7) || tb_odd_address(skin_w, w_f64 ? 7 : 3) || tb_odd_address(skin_idx, 3) ||
        tb_odd_address(rows, 7) || tb_odd_address(offsets, 7) || tb_odd_address(out, 3) || tb_odd_address(status, 3)) return D3GA_E_CONFIG;
    return 0;
}

}  // namespace d3ga
