// cage_author_math.h -- the rules of cage surface authoring (cage_author.hip): what the reference's
// cager/ops.py::cage_processor :140-148 does between a body mesh and the surface TetGen fills -- voxelise, fill, isosurface, two
// smoothers, connected components -- without trimesh, mcubes or open3d.  Compiles for the host as it is:
// tests/hostcheck/cage_author_host.cpp runs this very text on the CPU; cage_author.hip is compiled with -ffp-contract=off, so the device
// evaluates every expression here as g++ does.  Parity with trimesh, mcubes and open3d is UNPINNED: these rules are this library's.
//
// The grid.  D = 2 radius + 1 voxels per axis, pitch = 1 / (radius + 0.1).  Voxel (i,j,k) is the closed cube of side pitch centred at
//   ((i - r) pitch, (j - r) pitch, (k - r) pitch).  Bits are packed along x: word ((z D + y) W + (x >> 6)), bit x & 63, W = ceil(D / 64);
//   bits at x >= D are 0.
// 1 surface   voxel set iff a triangle meets its cube: the 13-axis separating-axis test on v_i = p_i - c, h = pitch / 2.  For an axis
//             a: p_i = (a.x v_i.x + a.y v_i.y) + a.z v_i.z, r = h ((|a.x| + |a.y|) + |a.z|); separated iff min p > r or max p < -r
//             (touching is meeting).  Axes in order: x, y, z; e_x x f_j, e_y x f_j, e_z x f_j for j = 0, 1, 2 with f_0 = v_1 - v_0,
//             f_1 = v_2 - v_1, f_2 = v_0 - v_2 (e_x x f = (0, -f.z, f.y), e_y x f = (f.z, 0, -f.x), e_z x f = (-f.y, f.x, 0)); f_0 x f_1.
//             A zero axis separates nothing, so a triangle without area is the segment or point it is.  The voxels tried for a
//             triangle are a superset of its box (one voxel of margin): the test alone decides.
// 2 fill      everything is occupied except the empty voxels 6-connected to the grid's border through empty voxels
//             (scipy.ndimage.binary_fill_holes).  outside starts as the empty border voxels; a round sweeps x (inside and across the
//             words of a row), then y, then z, each forward and back; rounds repeat until none changes a bit.  The fixed point is
//             unique; every sweep owns the words it writes, so the number of rounds is fixed too.
// 3 surface   marching tetrahedra on the grid padded with one empty layer.  Lattice point (px,py,pz), 0 <= p < P = D + 1, is grid
//             corner (px - 1, py - 1, pz - 1) and has linear index (pz P + py) P + px; it is the corner 0 of one cell, corners numbered
//             b = bx + 2 by + 4 bz, split into the six Kuhn tetrahedra {0, e_a, e_a | e_b, 7} in the order of kCaTet.  A crossed edge
//             (one end occupied) gives one vertex, its midpoint; the edge from lattice point q to q + offset has type 0..6 for offset
//             1, 2, 4, 3, 5, 6, 7 (x, y, z, xy, xz, yz, xyz).  Vertices ascend in (linear index of q, type); faces in (cell, tetrahedron,
//             table order).  Table: with `in` / `out` the tetrahedron's occupied / empty corners in its own order -- one corner s alone
//             on its side and o the other three: (s o0, s o1, s o2); two and two, in = (a, b), out = (c, d): (ac, ad, bd), (ac, bd, bc).
//             A triangle whose normal (p1 - p0) x (p2 - p0) points from `out` to `in` has its last two vertices swapped (integer test).
//             Grid coordinate x maps to ((x / radius - 1) + centre) / scale, one rounding to float32.
// 4 smoothing float64 positions, rounded to float32 once at the end; Jacobi: every iteration reads the previous positions.
//   improved  neighbours n ascending: w_n = 1 / |v - v_n|, s = sum w_n, m = sum (w_n / s) v_n, dot = m - v, N the angle-weighted
//             vertex normal (gauss_init_math.h rule 6), inner = (dot.x N.x + dot.y N.y) + dot.z N.z; inner >= 0: move = |dot| N, else
//             move = dot - inner N; v += lbd move.  A vertex of no face or no neighbour (STATUS_ISOLATED) and one with a neighbour
//             at distance 0 (STATUS_ZERO_EDGE) stay where they are.
//   taubin    v += f (sum v_n / k - v) with f = lambda, then f = mu, per iteration.
// 5 parts     faces sharing an edge are adjacent; label[f] = the smallest face index of f's part (min-label hooking of roots, then
//             pointer jumping, until no edge joins two roots: the fixed point is unique).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/d3ga.h"
#include "gauss_init_math.h"

namespace d3ga {

constexpr int kCaBlock = 256;
constexpr int32_t kCaMaxRadius = D3GA_CAGE_MAX_RADIUS;       // P = D + 1 = 1024: P^3 = 2^30 lattice points
constexpr int kCaTet[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};

D3GA_FHD int32_t ca_words(int32_t D) { return (D + 63) >> 6; }
D3GA_FHD double ca_pitch(int32_t radius) { return 1.0 / ((double)radius + 0.1); }
D3GA_FHD uint64_t ca_row_mask(int32_t D, int32_t w) { const int32_t left = D - 64 * w; return left >= 64 ? ~0ull : ((1ull << left) - 1ull); }
D3GA_FHD int64_t ca_word_at(int32_t D, int32_t W, int32_t w, int32_t y, int32_t z) { return ((int64_t)z * D + y) * W + w; }
D3GA_FHD int ca_occ(const uint64_t *bits, int32_t D, int32_t W, int32_t x, int32_t y, int32_t z) {
    if ((uint32_t)x >= (uint32_t)D || (uint32_t)y >= (uint32_t)D || (uint32_t)z >= (uint32_t)D) return 0;
    return (int)((bits[ca_word_at(D, W, x >> 6, y, z)] >> (x & 63)) & 1ull);
}

// ---- 1 surface ------------------------------------------------------------------------------------------------------------------------
D3GA_FHD bool ca_separates(double ax, double ay, double az, const double *v, double h) {
    const double p0 = (ax * v[0] + ay * v[1]) + az * v[2], p1 = (ax * v[3] + ay * v[4]) + az * v[5], p2 = (ax * v[6] + ay * v[7]) + az * v[8];
    const double r = h * ((fabs(ax) + fabs(ay)) + fabs(az));
    const double lo = p0 < p1 ? (p0 < p2 ? p0 : p2) : (p1 < p2 ? p1 : p2), hi = p0 > p1 ? (p0 > p2 ? p0 : p2) : (p1 > p2 ? p1 : p2);
    return lo > r || hi < -r;
}

// t: the triangle's nine coordinates; (cx, cy, cz) the cube's centre, h half its side
D3GA_FHD bool ca_tri_box(const double *t, double cx, double cy, double cz, double h) {
    double v[9];
    for (int i = 0; i < 3; ++i) { v[3 * i] = t[3 * i] - cx; v[3 * i + 1] = t[3 * i + 1] - cy; v[3 * i + 2] = t[3 * i + 2] - cz; }
    if (ca_separates(1.0, 0.0, 0.0, v, h) || ca_separates(0.0, 1.0, 0.0, v, h) || ca_separates(0.0, 0.0, 1.0, v, h)) return false;
    const double f[9] = {v[3] - v[0], v[4] - v[1], v[5] - v[2], v[6] - v[3], v[7] - v[4], v[8] - v[5], v[0] - v[6], v[1] - v[7], v[2] - v[8]};
    for (int j = 0; j < 3; ++j) {
        const double fx = f[3 * j], fy = f[3 * j + 1], fz = f[3 * j + 2];
        if (ca_separates(0.0, -fz, fy, v, h) || ca_separates(fz, 0.0, -fx, v, h) || ca_separates(-fy, fx, 0.0, v, h)) return false;
    }
    return !ca_separates(f[1] * f[5] - f[2] * f[4], f[2] * f[3] - f[0] * f[5], f[0] * f[4] - f[1] * f[3], v, h);
}

// the voxels tried along one axis for coordinates [lo, hi]: one more than the box on either side, cut to the grid
D3GA_FHD double ca_clampd(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }
D3GA_FHD int32_t ca_index_lo(double x, double pitch, int32_t r, int32_t D) {
    return (int32_t)ca_clampd(floor(ca_clampd(x / pitch, -2.0 * D, 2.0 * D) + (double)r + 0.5) - 1.0, 0.0, (double)D);
}
D3GA_FHD int32_t ca_index_hi(double x, double pitch, int32_t r, int32_t D) {
    return (int32_t)ca_clampd(floor(ca_clampd(x / pitch, -2.0 * D, 2.0 * D) + (double)r + 0.5) + 1.0, -1.0, (double)D - 1.0);
}

struct CaTriBox {
    double t[9];
    int32_t x0, y0, z0, nx, ny, nz;                          // first voxel and extent (0: nothing to try)
    bool bad;                                                // a face index outside [0, V) or a coordinate that is not finite
};
D3GA_FHD CaTriBox ca_tri_prepare(int32_t radius, int32_t V, const double *verts, const int32_t *face) {
    CaTriBox b;
    b.x0 = b.y0 = b.z0 = b.nx = b.ny = b.nz = 0;
    b.bad = false;
    for (int c = 0; c < 3; ++c) {
        if ((uint32_t)face[c] >= (uint32_t)V) { b.bad = true; return b; }
        for (int k = 0; k < 3; ++k) {
            const double x = verts[3 * (size_t)face[c] + k];
            if (!(fabs(x) <= 1e300)) { b.bad = true; return b; }
            b.t[3 * c + k] = x;
        }
    }
    const int32_t D = 2 * radius + 1;
    const double pitch = ca_pitch(radius);
    int32_t lo[3], hi[3];
    for (int k = 0; k < 3; ++k) {
        const double a = b.t[k], c = b.t[3 + k], d = b.t[6 + k];
        const double mn = a < c ? (a < d ? a : d) : (c < d ? c : d), mx = a > c ? (a > d ? a : d) : (c > d ? c : d);
        lo[k] = ca_index_lo(mn, pitch, radius, D);
        hi[k] = ca_index_hi(mx, pitch, radius, D);
        if (lo[k] > hi[k]) return b;
    }
    b.x0 = lo[0]; b.y0 = lo[1]; b.z0 = lo[2];
    b.nx = hi[0] - lo[0] + 1; b.ny = hi[1] - lo[1] + 1; b.nz = hi[2] - lo[2] + 1;
    return b;
}
// voxel i of the triangle's box (x fastest): true iff the triangle meets it; (x, y, z) receive the voxel
D3GA_FHD bool ca_tri_voxel(const CaTriBox &b, int32_t radius, int64_t i, int32_t *x, int32_t *y, int32_t *z) {
    *x = b.x0 + (int32_t)(i % b.nx);
    *y = b.y0 + (int32_t)((i / b.nx) % b.ny);
    *z = b.z0 + (int32_t)(i / ((int64_t)b.nx * b.ny));
    const double pitch = ca_pitch(radius);
    return ca_tri_box(b.t, (double)(*x - radius) * pitch, (double)(*y - radius) * pitch, (double)(*z - radius) * pitch, pitch / 2.0);
}

// ---- 2 fill ---------------------------------------------------------------------------------------------------------------------------
// every bit of `pro` reachable from a bit of `gen` through set bits of `pro`, within one word, both ways
D3GA_FHD uint64_t ca_flood_word(uint64_t gen, uint64_t pro) {
    uint64_t up = gen & pro, down = up, pu = pro, pd = pro;
    for (int k = 1; k < 64; k <<= 1) {
        up |= pu & (up << k);     pu &= pu << k;
        down |= pd & (down >> k); pd &= pd >> k;
    }
    return up | down;
}
// the empty border voxels of word (w, y, z)
D3GA_FHD uint64_t ca_border_word(const uint64_t *surface, int32_t D, int32_t W, int32_t w, int32_t y, int32_t z) {
    const uint64_t valid = ca_row_mask(D, w);
    uint64_t b = 0;
    if (y == 0 || y == D - 1 || z == 0 || z == D - 1) b = valid;
    if (w == 0) b |= 1ull;
    if (w == (D - 1) >> 6) b |= 1ull << ((D - 1) & 63);
    return b & valid & ~surface[ca_word_at(D, W, w, y, z)];
}
// one row (y, z): along x forward, then back.  Returns whether a bit was set.
D3GA_FHD bool ca_sweep_x(const uint64_t *surface, uint64_t *outside, int32_t D, int32_t W, int32_t y, int32_t z) {
    const int64_t base = ca_word_at(D, W, 0, y, z);
    bool changed = false;
    uint64_t carry = 0;
    for (int32_t w = 0; w < W; ++w) {
        const uint64_t pro = ~surface[base + w] & ca_row_mask(D, w), o = outside[base + w];
        const uint64_t n = o | ca_flood_word(o | carry, pro);
        if (n != o) { outside[base + w] = n; changed = true; }
        carry = n >> 63;
    }
    carry = 0;
    for (int32_t w = W - 1; w >= 0; --w) {
        const uint64_t pro = ~surface[base + w] & ca_row_mask(D, w), o = outside[base + w];
        const uint64_t n = o | ca_flood_word(o | (carry << 63), pro);
        if (n != o) { outside[base + w] = n; changed = true; }
        carry = n & 1ull;
    }
    return changed;
}
// D words `stride` apart from `start` (a column along y or z of one x word): forward, then back
D3GA_FHD bool ca_sweep_line(const uint64_t *surface, uint64_t *outside, int64_t start, int64_t stride, int32_t D, uint64_t valid) {
    bool changed = false;
    uint64_t prev = outside[start];
    for (int32_t i = 1; i < D; ++i) {
        const int64_t at = start + i * stride;
        const uint64_t o = outside[at], n = o | (prev & ~surface[at] & valid);
        if (n != o) { outside[at] = n; changed = true; }
        prev = n;
    }
    for (int32_t i = D - 2; i >= 0; --i) {
        const int64_t at = start + i * stride;
        const uint64_t o = outside[at], n = o | (prev & ~surface[at] & valid);
        if (n != o) { outside[at] = n; changed = true; }
        prev = n;
    }
    return changed;
}

// ---- 3 isosurface ---------------------------------------------------------------------------------------------------------------------
D3GA_FHD int ca_type_offset(int t) { return t < 2 ? t + 1 : (t == 2 ? 4 : (t == 3 ? 3 : t + 1)); }      // 1, 2, 4, 3, 5, 6, 7
D3GA_FHD int ca_offset_type(int off) { return off < 3 ? off - 1 : (off == 4 ? 2 : (off == 3 ? 3 : off - 1)); }

struct CaLattice { int32_t D, W, P; const uint64_t *bits; };
// the occupancy of the 8 corners of the cell whose corner 0 is lattice point (px, py, pz): bit b = corner b
D3GA_FHD int ca_corner_mask(const CaLattice &g, int32_t px, int32_t py, int32_t pz) {
    int m = 0;
    for (int b = 0; b < 8; ++b) m |= ca_occ(g.bits, g.D, g.W, px - 1 + (b & 1), py - 1 + ((b >> 1) & 1), pz - 1 + (b >> 2)) << b;
    return m;
}
// bit t: the edge of type t leaving corner 0 is crossed
D3GA_FHD int ca_cross_mask(int corner_mask) {
    int m = 0;
    for (int t = 0; t < 7; ++t) m |= (((corner_mask >> ca_type_offset(t)) ^ corner_mask) & 1) << t;
    return m;
}
D3GA_FHD int ca_popcount7(int m) { int n = 0; for (int t = 0; t < 7; ++t) n += (m >> t) & 1; return n; }
D3GA_FHD int ca_cell_faces(int corner_mask) {
    if (corner_mask == 0 || corner_mask == 255) return 0;
    int n = 0;
    for (int k = 0; k < 6; ++k) {
        const int in = ((corner_mask >> kCaTet[k][0]) & 1) + ((corner_mask >> kCaTet[k][1]) & 1) + ((corner_mask >> kCaTet[k][2]) & 1) + ((corner_mask >> kCaTet[k][3]) & 1);
        n += in == 2 ? 2 : (in == 1 || in == 3 ? 1 : 0);
    }
    return n;
}
// the triangles of tetrahedron k of a cell: tri[j][i] = {corner a, corner b} of the crossed edge that is vertex i; returns 0, 1 or 2
D3GA_FHD int ca_tet_triangles(int k, int corner_mask, int tri[2][3][2]) {
    int in[4], out[4], n_in = 0, n_out = 0;
    for (int i = 0; i < 4; ++i) {
        const int c = kCaTet[k][i];
        if ((corner_mask >> c) & 1) in[n_in++] = c; else out[n_out++] = c;
    }
    if (n_in == 0 || n_out == 0) return 0;
    int n = 1;
    if (n_in == 1 || n_out == 1) {
        const int s = n_in == 1 ? in[0] : out[0];
        const int *o = n_in == 1 ? out : in;
        for (int i = 0; i < 3; ++i) { tri[0][i][0] = s; tri[0][i][1] = o[i]; }
    } else {
        const int q[4][2] = {{in[0], out[0]}, {in[0], out[1]}, {in[1], out[1]}, {in[1], out[0]}};
        const int pick[2][3] = {{0, 1, 2}, {0, 2, 3}};
        for (int j = 0; j < 2; ++j)
            for (int i = 0; i < 3; ++i) { tri[j][i][0] = q[pick[j][i]][0]; tri[j][i][1] = q[pick[j][i]][1]; }
        n = 2;
    }
    int si[3] = {0, 0, 0}, so[3] = {0, 0, 0};                   // sums of the corners' coordinates
    for (int i = 0; i < n_in; ++i) { si[0] += in[i] & 1; si[1] += (in[i] >> 1) & 1; si[2] += in[i] >> 2; }
    for (int i = 0; i < n_out; ++i) { so[0] += out[i] & 1; so[1] += (out[i] >> 1) & 1; so[2] += out[i] >> 2; }
    for (int j = 0; j < n; ++j) {
        int p[3][3];                                         // twice the midpoints
        for (int i = 0; i < 3; ++i) {
            const int a = tri[j][i][0], b = tri[j][i][1];
            p[i][0] = (a & 1) + (b & 1); p[i][1] = ((a >> 1) & 1) + ((b >> 1) & 1); p[i][2] = (a >> 2) + (b >> 2);
        }
        const int u[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]}, w[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
        const int nrm[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
        int dot = 0;
        for (int c = 0; c < 3; ++c) dot += nrm[c] * (so[c] * n_in - si[c] * n_out);
        if (dot < 0) {
            const int a = tri[j][1][0], b = tri[j][1][1];
            tri[j][1][0] = tri[j][2][0]; tri[j][1][1] = tri[j][2][1];
            tri[j][2][0] = a; tri[j][2][1] = b;
        }
    }
    return n;
}

struct CaIsoMap { int32_t radius, reserved; double centre[3], scale[3]; };
// vertex (lattice point (px, py, pz), type t), coordinate c -> the output value
D3GA_FHD float ca_iso_coordinate(const CaIsoMap &m, int32_t p, int t, int c) {
    const double x = (double)(p - 1) + 0.5 * (double)((ca_type_offset(t) >> c) & 1);
    return (float)(((x / (double)m.radius - 1.0) + m.centre[c]) / m.scale[c]);
}
// the index of the vertex on the edge from corner a to corner b (a < b) of the cell at lattice point (px, py, pz)
D3GA_FHD int32_t ca_iso_vertex(const CaLattice &g, const uint32_t *vstart, int32_t px, int32_t py, int32_t pz, int a, int b) {
    const int32_t qx = px + (a & 1), qy = py + ((a >> 1) & 1), qz = pz + (a >> 2);
    if (qx >= g.P || qy >= g.P || qz >= g.P) return -1;     // never crossed: both ends lie in the padding
    const int t = ca_offset_type(b ^ a);
    const int cross = ca_cross_mask(ca_corner_mask(g, qx, qy, qz));
    return (int32_t)vstart[((int64_t)qz * g.P + qy) * g.P + qx] + ca_popcount7(cross & ((1 << t) - 1));
}
// the faces of the cell at lattice point (px, py, pz) -> out (3 n), returns n
D3GA_FHD int ca_cell_emit(const CaLattice &g, const uint32_t *vstart, int32_t px, int32_t py, int32_t pz, int corner_mask, int32_t *out) {
    int n = 0;
    for (int k = 0; k < 6; ++k) {
        int tri[2][3][2];
        const int m = ca_tet_triangles(k, corner_mask, tri);
        for (int j = 0; j < m; ++j, ++n)
            for (int i = 0; i < 3; ++i) {
                const int a = tri[j][i][0] < tri[j][i][1] ? tri[j][i][0] : tri[j][i][1], b = tri[j][i][0] < tri[j][i][1] ? tri[j][i][1] : tri[j][i][0];
                out[3 * n + i] = ca_iso_vertex(g, vstart, px, py, pz, a, b);
            }
    }
    return n;
}

// ---- 4 smoothing ----------------------------------------------------------------------------------------------------------------------
D3GA_FHD void ca_keep(const double *x, int32_t v, double *out) { out[0] = x[3 * (size_t)v]; out[1] = x[3 * (size_t)v + 1]; out[2] = x[3 * (size_t)v + 2]; }

D3GA_FHD void ca_improved_step(const d3ga_loop_plan &p, const double *x, const double *normals, int32_t v, double lbd, double *out, uint32_t *flags) {
    ca_keep(x, v, out);
    const int32_t begin = p.vert_offsets[v], end = p.vert_offsets[v + 1];
    if (end <= begin) { *flags |= D3GA_CAGE_STATUS_ISOLATED; return; }
    if (begin < 0 || (int64_t)end > 2 * (int64_t)p.E) { *flags |= D3GA_CAGE_STATUS_RANGE; return; }
    const GiVec xv = gi_vertex(x, v);
    double s = 0.0;
    for (int32_t j = begin; j < end; ++j) {
        const int32_t nb = p.vert_nbr[j];
        if ((uint32_t)nb >= (uint32_t)p.V) { *flags |= D3GA_CAGE_STATUS_RANGE; return; }
        const double d = gi_norm(gi_sub(xv, gi_vertex(x, nb)));
        if (!(d > 0.0)) { *flags |= D3GA_CAGE_STATUS_ZERO_EDGE; return; }
        s += 1.0 / d;
    }
    GiVec m = {0.0, 0.0, 0.0};
    for (int32_t j = begin; j < end; ++j) {
        const GiVec xn = gi_vertex(x, p.vert_nbr[j]);
        const double c = (1.0 / gi_norm(gi_sub(xv, xn))) / s;
        m.x += c * xn.x; m.y += c * xn.y; m.z += c * xn.z;
    }
    const GiVec dot = gi_sub(m, xv), N = gi_vertex(normals, v);
    const double inner = (dot.x * N.x + dot.y * N.y) + dot.z * N.z;
    GiVec move;
    if (inner >= 0.0) {
        const double H = sqrt((dot.x * dot.x + dot.y * dot.y) + dot.z * dot.z);
        move = {H * N.x, H * N.y, H * N.z};
    } else {
        move = {dot.x - inner * N.x, dot.y - inner * N.y, dot.z - inner * N.z};
    }
    out[0] = xv.x + lbd * move.x; out[1] = xv.y + lbd * move.y; out[2] = xv.z + lbd * move.z;
}

D3GA_FHD void ca_uniform_step(const d3ga_loop_plan &p, const double *x, int32_t v, double factor, double *out, uint32_t *flags) {
    ca_keep(x, v, out);
    const int32_t begin = p.vert_offsets[v], end = p.vert_offsets[v + 1];
    if (end <= begin) { *flags |= D3GA_CAGE_STATUS_ISOLATED; return; }
    if (begin < 0 || (int64_t)end > 2 * (int64_t)p.E) { *flags |= D3GA_CAGE_STATUS_RANGE; return; }
    GiVec m = {0.0, 0.0, 0.0};
    for (int32_t j = begin; j < end; ++j) {
        const int32_t nb = p.vert_nbr[j];
        if ((uint32_t)nb >= (uint32_t)p.V) { *flags |= D3GA_CAGE_STATUS_RANGE; return; }
        const GiVec xn = gi_vertex(x, nb);
        m.x += xn.x; m.y += xn.y; m.z += xn.z;
    }
    const double k = (double)(end - begin);
    out[0] += factor * (m.x / k - out[0]); out[1] += factor * (m.y / k - out[1]); out[2] += factor * (m.z / k - out[2]);
}

// the normal of vertex v for the improved step; a vertex of no face is flagged
D3GA_FHD void ca_normal(const GiMesh &m, const int32_t *csr_offsets, const int32_t *csr_faces, int32_t v, double *out, uint32_t *flags) {
    bool bad = false;
    if (csr_offsets[v + 1] <= csr_offsets[v]) *flags |= D3GA_CAGE_STATUS_ISOLATED;
    const GiVec n = gi_vertex_normal(m, csr_offsets, csr_faces, v, &bad);
    if (bad) *flags |= D3GA_CAGE_STATUS_RANGE;
    out[0] = n.x; out[1] = n.y; out[2] = n.z;
}

// ---- 5 parts --------------------------------------------------------------------------------------------------------------------------
// label[x] <= x always, so a chain of labels descends and ends at a root (label[r] == r) whatever other lanes store meanwhile
D3GA_FHD int32_t ca_root(const int32_t *label, int32_t f) {
    int32_t l = label[f];
    for (;;) {
        const int32_t n = label[l];
        if (n >= l) return l;
        l = n;
    }
}
// the two roots an edge joins: returns true (and larger / smaller) when they differ
D3GA_FHD bool ca_edge_roots(const d3ga_loop_plan &p, const int32_t *label, int32_t e, int32_t *larger, int32_t *smaller) {
    const int32_t f0 = p.edge_faces[2 * (size_t)e], f1 = p.edge_faces[2 * (size_t)e + 1];
    if ((uint32_t)f0 >= (uint32_t)p.F || (uint32_t)f1 >= (uint32_t)p.F) return false;
    const int32_t a = ca_root(label, f0), b = ca_root(label, f1);
    if (a == b) return false;
    *larger = a > b ? a : b;
    *smaller = a > b ? b : a;
    return true;
}

// ---- scratch layout of the isosurface and the argument rules of the entry points (include/d3ga.h); nothing is dereferenced ------------
//   [0] vstart       N uint32    the number of the first vertex of every lattice point, N = P^3
//   [1] block_total  2 nblk uint32   vertices, then faces, of every block of kCaBlock lattice points
//   [2] block_start  2 (nblk + 1) uint64
static inline int64_t ca_align256(int64_t x) { return (x + 255) & ~int64_t(255); }
static inline int64_t ca_lattice_points(int32_t radius) { const int64_t P = 2 * (int64_t)radius + 2; return P * P * P; }
static inline int64_t ca_blocks(int64_t n) { return (n + kCaBlock - 1) / kCaBlock; }
static inline int64_t ca_iso_scratch_bytes(int32_t radius) {
    const int64_t N = ca_lattice_points(radius), nb = ca_blocks(N);
    return ca_align256(4 * N) + ca_align256(8 * nb) + ca_align256(16 * (nb + 1));
}
struct CaIsoScratch { uint32_t *vstart, *total_v, *total_f; uint64_t *start_v, *start_f; };
static inline CaIsoScratch ca_iso_carve(void *base, int32_t radius) {
    const int64_t N = ca_lattice_points(radius), nb = ca_blocks(N);
    char *p = static_cast<char *>(base);
    CaIsoScratch s;
    s.vstart = reinterpret_cast<uint32_t *>(p);   p += ca_align256(4 * N);
    s.total_v = reinterpret_cast<uint32_t *>(p);  s.total_f = s.total_v + nb;  p += ca_align256(8 * nb);
    s.start_v = reinterpret_cast<uint64_t *>(p);  s.start_f = s.start_v + (nb + 1);
    return s;
}

static inline bool ca_odd(const void *p, uintptr_t mask) { return ((uintptr_t)p & mask) != 0; }
static inline int ca_check_grid(const d3ga_voxel_grid *g) {
    if (!g) return D3GA_E_NULL;
    if (g->radius < 1 || g->radius > kCaMaxRadius || g->D != 2 * g->radius + 1 || g->W != ca_words(g->D)) return D3GA_E_SIZE;
    if (!g->bits) return D3GA_E_NULL;
    if (ca_odd(g->bits, 7)) return D3GA_E_CONFIG;
    return 0;
}
static inline int ca_check_voxelize(const d3ga_voxel_grid *g, int32_t V, int32_t F, const double *verts, const int32_t *faces, const uint32_t *status) {
    const int st = ca_check_grid(g);
    if (st != 0) return st;
    if (V <= 0 || F <= 0 || 3 * (int64_t)V > INT32_MAX || 3 * (int64_t)F > INT32_MAX) return D3GA_E_SIZE;
    if (!verts || !faces || !status) return D3GA_E_NULL;
    if (ca_odd(verts, 7) || ca_odd(faces, 3) || ca_odd(status, 3)) return D3GA_E_CONFIG;
    return 0;
}
static inline int ca_check_fill(const d3ga_voxel_grid *g, int32_t stage, const uint64_t *outside, const uint64_t *filled, const int32_t *changed) {
    const int st = ca_check_grid(g);
    if (st != 0) return st;
    if (stage < D3GA_CAGE_FILL_BEGIN || stage > D3GA_CAGE_FILL_FINISH) return D3GA_E_CONFIG;
    if (!outside || (stage == D3GA_CAGE_FILL_ROUND && !changed) || (stage == D3GA_CAGE_FILL_FINISH && !filled)) return D3GA_E_NULL;
    if (ca_odd(outside, 7) || ca_odd(filled, 7) || ca_odd(changed, 3)) return D3GA_E_CONFIG;
    if (outside == g->bits || filled == g->bits) return D3GA_E_CONFIG;
    return 0;
}
static inline int ca_check_iso_count(const d3ga_voxel_grid *g, const void *scratch, int64_t scratch_bytes, const int64_t *counts) {
    const int st = ca_check_grid(g);
    if (st != 0) return st;
    if (!scratch || !counts) return D3GA_E_NULL;
    if (ca_odd(scratch, 255) || ca_odd(counts, 7)) return D3GA_E_CONFIG;
    if (scratch_bytes < ca_iso_scratch_bytes(g->radius)) return D3GA_E_CAPACITY;
    return 0;
}
static inline int ca_check_iso_emit(const d3ga_voxel_grid *g, const d3ga_cage_iso_desc *o, const void *scratch, int64_t scratch_bytes) {
    if (!o) return D3GA_E_NULL;
    const int st = ca_check_iso_count(g, scratch, scratch_bytes, reinterpret_cast<const int64_t *>(scratch));
    if (st != 0) return st;
    if (o->n_vertices <= 0 || o->n_faces <= 0 || 3 * (int64_t)o->n_vertices > INT32_MAX || 3 * (int64_t)o->n_faces > INT32_MAX) return D3GA_E_SIZE;
    if (!o->vertices || !o->faces) return D3GA_E_NULL;
    if (ca_odd(o->vertices, 3) || ca_odd(o->faces, 3)) return D3GA_E_CONFIG;
    for (int c = 0; c < 3; ++c)
        if (!(fabs(o->centre[c]) <= 1e300) || !(fabs(o->scale[c]) <= 1e300) || !(fabs(o->scale[c]) >= 1e-300)) return D3GA_E_CONFIG;
    return 0;
}
static inline int ca_check_plan(const d3ga_loop_plan *p) {
    if (!p) return D3GA_E_NULL;
    if (p->V <= 0 || p->F <= 0 || p->E <= 0 || 6 * (int64_t)p->F > INT32_MAX || p->E > 3 * (int64_t)p->F || 3 * (int64_t)p->V > INT32_MAX) return D3GA_E_SIZE;
    if (!p->edge_faces || !p->vert_offsets || !p->vert_nbr) return D3GA_E_NULL;
    if (ca_odd(p->edge_faces, 3) || ca_odd(p->vert_offsets, 3) || ca_odd(p->vert_nbr, 3)) return D3GA_E_CONFIG;
    return 0;
}
static inline int ca_check_smooth(const d3ga_loop_plan *p, const d3ga_cage_smooth_desc *s) {
    if (!s) return D3GA_E_NULL;
    const int st = ca_check_plan(p);
    if (st != 0) return st;
    if (s->iterations < 1 || s->iterations > D3GA_CAGE_MAX_ITERATIONS) return D3GA_E_SIZE;
    if (s->mode != D3GA_CAGE_SMOOTH_IMPROVED && s->mode != D3GA_CAGE_SMOOTH_TAUBIN) return D3GA_E_CONFIG;
    if (!(fabs(s->lam) <= 1e300) || !(fabs(s->mu) <= 1e300)) return D3GA_E_CONFIG;
    if (!s->x || !s->work || !s->out || !s->status) return D3GA_E_NULL;
    if (s->mode == D3GA_CAGE_SMOOTH_IMPROVED && (!s->faces || !s->csr_offsets || !s->csr_faces || !s->normals)) return D3GA_E_NULL;
    if (ca_odd(s->x, 7) || ca_odd(s->work, 7) || ca_odd(s->normals, 7) || ca_odd(s->out, 3) || ca_odd(s->status, 3) || ca_odd(s->faces, 3) ||
        ca_odd(s->csr_offsets, 3) || ca_odd(s->csr_faces, 3)) return D3GA_E_CONFIG;
    if (s->work == s->x || s->normals == s->x || s->normals == s->work) return D3GA_E_CONFIG;
    return 0;
}
static inline int ca_check_components(const d3ga_loop_plan *p, int32_t stage, const int32_t *label, const int32_t *changed) {
    const int st = ca_check_plan(p);
    if (st != 0) return st;
    if (stage != D3GA_CAGE_PARTS_BEGIN && stage != D3GA_CAGE_PARTS_ROUND) return D3GA_E_CONFIG;
    if (!label || (stage == D3GA_CAGE_PARTS_ROUND && !changed)) return D3GA_E_NULL;
    if (ca_odd(label, 3) || ca_odd(changed, 3)) return D3GA_E_CONFIG;
    return 0;
}

}  // namespace d3ga
