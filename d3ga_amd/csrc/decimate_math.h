// decimate_math.h -- the rules of quadric edge-collapse decimation (decimate.hip): what the reference's
// cager/ops.py::simplify :121-137 asks of open3d's simplify_quadric_decimation, as rounds of independent collapses.  Compiles for the
// host as it is: tests/hostcheck/decimate_host.cpp runs this very text on the CPU; decimate.hip is compiled with -ffp-contract=off, so
// the device evaluates every expression here as g++ does.  Parity with open3d's serial priority queue is UNPINNED: these rules are this
// library's.  A last-bit difference in a cost can change which edge wins, so every sum below has ONE order, the one written.
//
// State   float64 positions x (V,3), one symmetric 4x4 quadric per vertex as 10 float64 in the order xx xy xz xw yy yz yw zz zw ww,
//         int32 faces.  Vertices are never renumbered between rounds: a vanished vertex is no longer named by a face.
// 1 quadrics  face (a,b,c): n = (b - a) x (c - a) (gi_cross), len = sqrt((n.x n.x + n.y n.y) + n.z n.z), area = len / 2, m = n / len
//         per component, p = (m.x, m.y, m.z, -((m.x a.x + m.y a.y) + m.z a.z)), K_ij = area (p_i p_j).  Q[v] = 0 + K + K + ... over the
//         faces of v in ascending face index.  A face with len = 0 (or not a number) adds nothing.
// 2 round     the caller builds the d3ga_loop_plan of the current faces and the vertex -> face lists; need = ceil((F - target) / 2).
// 3 edge e = (u, w), u < w; u survives.  Valid iff
//     (a) neither end is a boundary vertex;
//     (b) the ascending neighbour lists of u and w, merged, have exactly two common entries, and they are the edge's opposite
//         vertices a, b;
//     (c) not (a face of u names both a and b, and a face of w names both a and b): the edge a-b would then have u and w as its
//         opposite vertices and the two remaining faces would coincide (the tetrahedron);
//     (d) q = Q[u] + Q[w] per entry; A = the upper 3x3, r = -(q.xw, q.yw, q.zw).  With
//           m00 = yy zz - yz yz, m01 = xy zz - yz xz, m02 = xy yz - yy xz, det = (xx m00 - xy m01) + xz m02,
//         if |det| > 1e-10 (amax amax) amax, amax the largest |entry| of A, the point is adj(A) r / det:
//           ((i_k0 r0 + i_k1 r1) + i_k2 r2) / det with i00 = m00, i01 = xz yz - xy zz, i02 = m02, i11 = xx zz - xz xz,
//           i12 = xy xz - xx yz, i22 = xx yy - xy xy.
//         Otherwise it is whichever of x[u], x[w], (x[u] + x[w]) 0.5 has the smallest cost, ties in that order.  cost(p) =
//           ((x t0 + y t1) + z t2) + t3, t_i = ((q_i0 x + q_i1 y) + q_i2 z) + q_i3; a negative cost counts as 0.  A point whose cost
//         is not finite is never chosen, and the edge is invalid when no point is left;
//     (e) for every face of u and of w that does not name both ends: old normal n = (p1 - p0) x (p2 - p0), new normal n' with the end
//         at the chosen point; (n.x n'.x + n.y n'.y) + n.z n'.z > 0.  A face with n = 0 is skipped.
//     key = (bits of (float)min(cost, FLT_MAX)) << 32 | e: positive, smaller is better; an invalid edge has D3GA_LOOP_BAD_KEY.
// 4 admission the keys are sorted ascending; the first `need` valid ones are admitted.
// 5 selection every admitted edge does atomicMin(owner[u], key), atomicMin(owner[w], key) (64-bit integers, cells start at all
//         ones); it is selected iff owner[t] >= key for every t in {u, w} + N[u] + N[w].
// 6 apply     per selected edge x[u] = the point, Q[u] = Q[u] + Q[w] per entry, remap[w] = u.  Per face: every corner through remap;
//         a face that now names a vertex twice is dropped, the others keep their order and their winding.
// 7 end       the caller stops at need <= 0; a round without a valid edge or the round limit sets D3GA_CAGE_STATUS_STUCK.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/d3ga.h"
#include "cage_author_math.h"

namespace d3ga {

constexpr int kDcBlock = 256;
constexpr int64_t kDcBadKey = D3GA_LOOP_BAD_KEY;
constexpr uint64_t kDcNoOwner = ~0ull;
constexpr double kDcFloatMax = 3.4028234663852886e38, kDcDoubleMax = 1.7976931348623157e308;

struct DcMesh {
    int32_t V, F;
    const double *x, *Q;
    const int32_t *faces, *csr_offsets, *csr_faces;
};

// ---- 1 quadrics -----------------------------------------------------------------------------------------------------------------------
D3GA_FHD bool dc_face_quadric(GiVec a, GiVec b, GiVec c, double *K) {
    const GiVec n = gi_cross(gi_sub(b, a), gi_sub(c, a));
    const double len = sqrt((n.x * n.x + n.y * n.y) + n.z * n.z);
    if (!(len > 0.0)) return false;
    const double area = len / 2.0;
    const GiVec m = {n.x / len, n.y / len, n.z / len};
    const double p[4] = {m.x, m.y, m.z, -((m.x * a.x + m.y * a.y) + m.z * a.z)};
    int k = 0;
    for (int i = 0; i < 4; ++i)
        for (int j = i; j < 4; ++j) K[k++] = area * (p[i] * p[j]);
    return true;
}

// the corners of face f, or false (and the range bit) for an index outside its table
D3GA_FHD bool dc_face(const DcMesh &m, int32_t f, int32_t *i, uint32_t *flags) {
    if ((uint32_t)f >= (uint32_t)m.F) { *flags |= D3GA_CAGE_STATUS_RANGE; return false; }
    for (int c = 0; c < 3; ++c) {
        i[c] = m.faces[3 * (size_t)f + c];
        if ((uint32_t)i[c] >= (uint32_t)m.V) { *flags |= D3GA_CAGE_STATUS_RANGE; return false; }
    }
    return true;
}
// the range [begin, end) of the faces of v in csr_faces, or false
D3GA_FHD bool dc_star(const DcMesh &m, int32_t v, int32_t *begin, int32_t *end, uint32_t *flags) {
    *begin = m.csr_offsets[v];
    *end = m.csr_offsets[v + 1];
    if (*begin < 0 || *end < *begin || (int64_t)*end > 3 * (int64_t)m.F) { *flags |= D3GA_CAGE_STATUS_RANGE; return false; }
    return true;
}

D3GA_FHD void dc_vertex_quadric(const DcMesh &m, int32_t v, double *out, uint32_t *flags) {
    for (int k = 0; k < 10; ++k) out[k] = 0.0;
    int32_t begin, end, i[3];
    if (!dc_star(m, v, &begin, &end, flags)) return;
    for (int32_t j = begin; j < end; ++j) {
        if (!dc_face(m, m.csr_faces[j], i, flags)) continue;
        double K[10];
        if (!dc_face_quadric(gi_vertex(m.x, i[0]), gi_vertex(m.x, i[1]), gi_vertex(m.x, i[2]), K)) continue;
        for (int k = 0; k < 10; ++k) out[k] += K[k];
    }
}

// ---- 3 (d) placement ------------------------------------------------------------------------------------------------------------------
// the cost of a point, negative values as 0; +infinity for a cost that is not finite
D3GA_FHD double dc_cost(const double *q, GiVec p) {
    const double t0 = ((q[0] * p.x + q[1] * p.y) + q[2] * p.z) + q[3];
    const double t1 = ((q[1] * p.x + q[4] * p.y) + q[5] * p.z) + q[6];
    const double t2 = ((q[2] * p.x + q[5] * p.y) + q[7] * p.z) + q[8];
    const double t3 = ((q[3] * p.x + q[6] * p.y) + q[8] * p.z) + q[9];
    const double c = ((p.x * t0 + p.y * t1) + p.z * t2) + t3;
    if (!(fabs(c) <= kDcDoubleMax)) return INFINITY;
    return c > 0.0 ? c : 0.0;
}

D3GA_FHD double dc_max2(double a, double b) { return a > b ? a : b; }

// the point the edge collapses to and its cost; false when no point has a finite cost
D3GA_FHD bool dc_place(const double *q, GiVec xu, GiVec xw, GiVec *point, double *cost) {
    const double xx = q[0], xy = q[1], xz = q[2], yy = q[4], yz = q[5], zz = q[7];
    const double amax = dc_max2(dc_max2(dc_max2(fabs(xx), fabs(xy)), dc_max2(fabs(xz), fabs(yy))), dc_max2(fabs(yz), fabs(zz)));
    const double m00 = yy * zz - yz * yz, m01 = xy * zz - yz * xz, m02 = xy * yz - yy * xz;
    const double det = (xx * m00 - xy * m01) + xz * m02;
    if (fabs(det) > 1e-10 * ((amax * amax) * amax)) {
        const double i01 = xz * yz - xy * zz, i11 = xx * zz - xz * xz, i12 = xy * xz - xx * yz, i22 = xx * yy - xy * xy;
        const double r0 = -q[3], r1 = -q[6], r2 = -q[8];
        *point = {((m00 * r0 + i01 * r1) + m02 * r2) / det, ((i01 * r0 + i11 * r1) + i12 * r2) / det, ((m02 * r0 + i12 * r1) + i22 * r2) / det};
        *cost = dc_cost(q, *point);
        return *cost < INFINITY;
    }
    const GiVec mid = {(xu.x + xw.x) * 0.5, (xu.y + xw.y) * 0.5, (xu.z + xw.z) * 0.5};
    const double cu = dc_cost(q, xu), cw = dc_cost(q, xw), cm = dc_cost(q, mid);
    *point = xu;
    *cost = cu;
    if (cw < *cost) { *point = xw; *cost = cw; }
    if (cm < *cost) { *point = mid; *cost = cm; }
    return *cost < INFINITY;
}

D3GA_FHD int64_t dc_key(double cost, int32_t e) {
    const float c = (float)(cost > kDcFloatMax ? kDcFloatMax : cost);
    uint32_t bits;
    memcpy(&bits, &c, 4);
    return (int64_t)(((uint64_t)bits << 32) | (uint32_t)e);
}
D3GA_FHD int32_t dc_key_edge(int64_t key) { return (int32_t)(key & 0xffffffffll); }

// ---- 3 (b) the link condition on vertices ---------------------------------------------------------------------------------------------
// the range of the neighbours of v in vert_nbr, or false
D3GA_FHD bool dc_ring(const d3ga_loop_plan &p, int32_t v, int32_t *begin, int32_t *end, uint32_t *flags) {
    *begin = p.vert_offsets[v];
    *end = p.vert_offsets[v + 1];
    if (*begin < 0 || *end < *begin || (int64_t)*end > 2 * (int64_t)p.E) { *flags |= D3GA_CAGE_STATUS_RANGE; return false; }
    return true;
}
// the number of common neighbours of u and w (the first two in c), by a merge of the two ascending lists; -1: a table out of range
D3GA_FHD int dc_common(const d3ga_loop_plan &p, int32_t u, int32_t w, int32_t *c, uint32_t *flags) {
    int32_t i, iend, j, jend;
    if (!dc_ring(p, u, &i, &iend, flags) || !dc_ring(p, w, &j, &jend, flags)) return -1;
    int n = 0;
    while (i < iend && j < jend) {
        const int32_t a = p.vert_nbr[i], b = p.vert_nbr[j];
        if (a < b) ++i;
        else if (b < a) ++j;
        else {
            if (n < 2) c[n] = a;
            ++n; ++i; ++j;
        }
    }
    return n;
}

// ---- 3 (c), (e): one end's faces ------------------------------------------------------------------------------------------------------
// the faces of `end` that do not name `other`: false if one of them flips with `end` at `point`; *shared: one of them names a and b
D3GA_FHD bool dc_star_keeps(const DcMesh &m, int32_t end, int32_t other, int32_t a, int32_t b, GiVec point, bool *shared, uint32_t *flags) {
    int32_t begin, stop, i[3];
    *shared = false;
    if (!dc_star(m, end, &begin, &stop, flags)) return false;
    bool ok = true;
    for (int32_t j = begin; j < stop; ++j) {
        if (!dc_face(m, m.csr_faces[j], i, flags)) { ok = false; continue; }
        if (i[0] == other || i[1] == other || i[2] == other) continue;
        if ((i[0] == a || i[1] == a || i[2] == a) && (i[0] == b || i[1] == b || i[2] == b)) *shared = true;
        GiVec p[3], r[3];
        for (int c = 0; c < 3; ++c) {
            p[c] = gi_vertex(m.x, i[c]);
            r[c] = i[c] == end ? point : p[c];
        }
        const GiVec n = gi_cross(gi_sub(p[1], p[0]), gi_sub(p[2], p[0]));
        if (n.x == 0.0 && n.y == 0.0 && n.z == 0.0) continue;
        const GiVec t = gi_cross(gi_sub(r[1], r[0]), gi_sub(r[2], r[0]));
        if (!((n.x * t.x + n.y * t.y) + n.z * t.z > 0.0)) ok = false;
    }
    return ok;
}

// ---- 3 the key of edge e and the point it collapses to --------------------------------------------------------------------------------
D3GA_FHD int64_t dc_candidate(const d3ga_loop_plan &p, const DcMesh &m, int32_t e, double *point_out, uint32_t *flags) {
    point_out[0] = point_out[1] = point_out[2] = 0.0;
    const int32_t u = p.edge_verts[2 * (size_t)e], w = p.edge_verts[2 * (size_t)e + 1];
    if ((uint32_t)u >= (uint32_t)p.V || (uint32_t)w >= (uint32_t)p.V || u >= w) { *flags |= D3GA_CAGE_STATUS_RANGE; return kDcBadKey; }
    if (p.edge_boundary[e] || p.vert_boundary[u] || p.vert_boundary[w]) return kDcBadKey;                   // (a)
    const int32_t a = p.edge_opp[2 * (size_t)e], b = p.edge_opp[2 * (size_t)e + 1];
    if ((uint32_t)a >= (uint32_t)p.V || (uint32_t)b >= (uint32_t)p.V) { *flags |= D3GA_CAGE_STATUS_RANGE; return kDcBadKey; }
    int32_t c[2] = {-1, -1};
    if (dc_common(p, u, w, c, flags) != 2) return kDcBadKey;                                                // (b)
    if (!((c[0] == a && c[1] == b) || (c[0] == b && c[1] == a))) return kDcBadKey;
    double q[10];
    for (int k = 0; k < 10; ++k) q[k] = m.Q[10 * (size_t)u + k] + m.Q[10 * (size_t)w + k];
    GiVec point;
    double cost;
    if (!dc_place(q, gi_vertex(m.x, u), gi_vertex(m.x, w), &point, &cost)) return kDcBadKey;                // (d)
    bool shared_u, shared_w;
    const bool keeps_u = dc_star_keeps(m, u, w, a, b, point, &shared_u, flags), keeps_w = dc_star_keeps(m, w, u, a, b, point, &shared_w, flags);
    if (!keeps_u || !keeps_w) return kDcBadKey;                                                             // (e)
    if (shared_u && shared_w) return kDcBadKey;                                                             // (c)
    point_out[0] = point.x; point_out[1] = point.y; point_out[2] = point.z;
    return dc_key(cost, e);
}

// ---- 5 selection ----------------------------------------------------------------------------------------------------------------------
// the ends of the admitted edge at rank i of the sorted keys, or false for an invalid key
D3GA_FHD bool dc_admitted(const d3ga_loop_plan &p, const int64_t *sorted_keys, int32_t i, int64_t *key, int32_t *u, int32_t *w, uint32_t *flags) {
    *key = sorted_keys[i];
    if (*key == kDcBadKey || *key < 0) return false;
    const int32_t e = dc_key_edge(*key);
    if ((uint32_t)e >= (uint32_t)p.E) { *flags |= D3GA_CAGE_STATUS_RANGE; return false; }
    *u = p.edge_verts[2 * (size_t)e];
    *w = p.edge_verts[2 * (size_t)e + 1];
    if ((uint32_t)*u >= (uint32_t)p.V || (uint32_t)*w >= (uint32_t)p.V) { *flags |= D3GA_CAGE_STATUS_RANGE; return false; }
    return true;
}
D3GA_FHD bool dc_ring_free(const d3ga_loop_plan &p, const uint64_t *owner, int32_t v, uint64_t key, uint32_t *flags) {
    int32_t begin, end;
    if (owner[v] < key || !dc_ring(p, v, &begin, &end, flags)) return false;
    for (int32_t j = begin; j < end; ++j) {
        const int32_t t = p.vert_nbr[j];
        if ((uint32_t)t >= (uint32_t)p.V) { *flags |= D3GA_CAGE_STATUS_RANGE; return false; }
        if (owner[t] < key) return false;
    }
    return true;
}
D3GA_FHD bool dc_selected(const d3ga_loop_plan &p, const uint64_t *owner, int32_t u, int32_t w, int64_t key, uint32_t *flags) {
    return dc_ring_free(p, owner, u, (uint64_t)key, flags) && dc_ring_free(p, owner, w, (uint64_t)key, flags);
}

// ---- 6 apply --------------------------------------------------------------------------------------------------------------------------
D3GA_FHD void dc_apply(double *x, double *Q, int32_t *remap, int32_t u, int32_t w, const double *point) {
    for (int c = 0; c < 3; ++c) x[3 * (size_t)u + c] = point[c];
    for (int k = 0; k < 10; ++k) Q[10 * (size_t)u + k] = Q[10 * (size_t)u + k] + Q[10 * (size_t)w + k];
    remap[w] = u;
}
// face f through remap -> out; false for a face that is dropped
D3GA_FHD bool dc_relabel(int32_t V, const int32_t *faces, const int32_t *remap, int32_t f, int32_t *out, uint32_t *flags) {
    for (int c = 0; c < 3; ++c) {
        const int32_t v = faces[3 * (size_t)f + c];
        if ((uint32_t)v >= (uint32_t)V) { *flags |= D3GA_CAGE_STATUS_RANGE; return false; }
        out[c] = remap[v];
        if ((uint32_t)out[c] >= (uint32_t)V) { *flags |= D3GA_CAGE_STATUS_RANGE; return false; }
    }
    return out[0] != out[1] && out[1] != out[2] && out[2] != out[0];
}

// ---- scratch of the face compaction and the argument rules of the entry points (include/d3ga.h); nothing is dereferenced ---------------
//   [0] block_total  nblk uint32      kept faces of every block of kDcBlock faces
//   [1] block_start  (nblk + 1) uint64
static inline int64_t dc_blocks(int64_t n) { return (n + kDcBlock - 1) / kDcBlock; }
static inline int64_t dc_scratch_bytes(int32_t F) { return ca_align256(4 * dc_blocks(F)) + ca_align256(8 * (dc_blocks(F) + 1)); }
struct DcScratch { uint32_t *block_total; uint64_t *block_start; };
static inline DcScratch dc_carve(void *base, int32_t F) {
    char *p = static_cast<char *>(base);
    DcScratch s;
    s.block_total = reinterpret_cast<uint32_t *>(p);  p += ca_align256(4 * dc_blocks(F));
    s.block_start = reinterpret_cast<uint64_t *>(p);
    return s;
}

static inline int dc_check_plan(const d3ga_loop_plan *p, const d3ga_decimate_desc *d) {
    if (!d) return D3GA_E_NULL;
    const int st = ca_check_plan(p);
    if (st != 0) return st;
    if (!p->edge_verts || !p->edge_opp || !p->edge_boundary || !p->vert_boundary) return D3GA_E_NULL;
    if (ca_odd(p->edge_verts, 3) || ca_odd(p->edge_opp, 3)) return D3GA_E_CONFIG;
    return 0;
}
static inline int dc_check_mesh(const d3ga_decimate_desc *d) {
    if (!d->x || !d->quadrics || !d->faces || !d->csr_offsets || !d->csr_faces || !d->status) return D3GA_E_NULL;
    if (ca_odd(d->x, 7) || ca_odd(d->quadrics, 7) || ca_odd(d->faces, 3) || ca_odd(d->csr_offsets, 3) || ca_odd(d->csr_faces, 3) || ca_odd(d->status, 3))
        return D3GA_E_CONFIG;
    return 0;
}
static inline int dc_check_quadrics(const d3ga_loop_plan *p, const d3ga_decimate_desc *d) {
    const int st = dc_check_plan(p, d);
    return st != 0 ? st : dc_check_mesh(d);
}
static inline int dc_check_candidates(const d3ga_loop_plan *p, const d3ga_decimate_desc *d) {
    int st = dc_check_plan(p, d);
    if (st == 0) st = dc_check_mesh(d);
    if (st != 0) return st;
    if (!d->keys || !d->placement || !d->owner || !d->remap || !d->counts) return D3GA_E_NULL;
    if (ca_odd(d->keys, 7) || ca_odd(d->placement, 7) || ca_odd(d->owner, 7) || ca_odd(d->remap, 3) || ca_odd(d->counts, 7)) return D3GA_E_CONFIG;
    return 0;
}
static inline int dc_check_collapse(const d3ga_loop_plan *p, const d3ga_decimate_desc *d) {
    const int st = dc_check_plan(p, d);
    if (st != 0) return st;
    if (d->n_admit < 1 || d->n_admit > p->E) return D3GA_E_SIZE;
    if (!d->x || !d->quadrics || !d->placement || !d->sorted_keys || !d->owner || !d->remap || !d->status) return D3GA_E_NULL;
    if (ca_odd(d->x, 7) || ca_odd(d->quadrics, 7) || ca_odd(d->placement, 7) || ca_odd(d->sorted_keys, 7) || ca_odd(d->owner, 7) || ca_odd(d->remap, 3) ||
        ca_odd(d->status, 3)) return D3GA_E_CONFIG;
    return 0;
}
static inline int dc_check_faces(const d3ga_loop_plan *p, const d3ga_decimate_desc *d) {
    const int st = dc_check_plan(p, d);
    if (st != 0) return st;
    if (!d->faces || !d->faces_out || !d->remap || !d->scratch || !d->counts || !d->status) return D3GA_E_NULL;
    if (ca_odd(d->faces, 3) || ca_odd(d->faces_out, 3) || ca_odd(d->remap, 3) || ca_odd(d->scratch, 255) || ca_odd(d->counts, 7) || ca_odd(d->status, 3) ||
        d->faces_out == d->faces) return D3GA_E_CONFIG;
    if (d->scratch_bytes < dc_scratch_bytes(p->F)) return D3GA_E_CAPACITY;
    return 0;
}

}  // namespace d3ga
