// gauss_init_math.h -- the rules of Gaussian initialisation (gauss_init.hip): what the reference's
// lib/cage.py::CageBase.sample_initial_points :262-296 does between a mesh and (points, rotations, faces, barys) -- trimesh's
// sample_surface, the TBN frame, pytorch3d's matrix_to_quaternion, compute_tris_bary :241-260 -- and the angle-weighted vertex
// normals behind `mesh.vertex_normals * inflate` :271-272.  Compiles for the host as it is: tests/hostcheck/gauss_init_host.cpp runs
// this very text on the CPU against tests/gauss_init_ref.py; gauss_init.hip is compiled with -ffp-contract=off, so the device
// evaluates every expression here as g++ does (fp64 division and square root are correctly rounded on both).
//
// All arithmetic is float64 with ONE rounding to float32 per output element.  Inputs: vertices (V,3) float64, faces (F,3) int32,
// an optional face mask (F) of bytes, uniforms (n,3) float64 in [0,1).
//   1 weights   area_f = 0.5 |e0 x e1|, e0 = v1 - v0, e1 = v2 - v0; 0 for a masked-out face, a face that names a vertex outside
//               [0, V) (status D3GA_SAMPLE_STATUS_RANGE) and an area that is not finite.  E: max area < 2^E, from the bits of the
//               maximum (an integer maximum: exact, any order).  k = 62 - E - ceil(log2 F).  q_f = floor(area_f 2^k) as uint64,
//               taken from the double's mantissa by a shift.  cum = inclusive integer prefix sum of q, total = cum[F-1] < 2^62.
//               Stored as cum_local (inclusive within blocks of kGiBlock faces) + block_start (exclusive prefix of the block totals).
//   2 face      m = floor(u0 2^53); pick = (m total) >> 53 (128-bit product); face = the first i with cum[i] > pick.
//   3 point     (r1, r2) = (u1, u2); r1 + r2 > 1: each becomes |r - 1|.  p = v0 + r1 e0 + r2 e1.
//   4 frame     N = normalize(e0 x e1), T = normalize(e0 x N), B = normalize(e0 x T), normalize = x / max(|x|, 1e-12); the matrix
//               with columns T, B, N -> quaternion wxyz by pytorch3d's matrix_to_quaternion rule.
//   5 barys     from the FLOAT32-rounded point promoted back: v = (d11 d20 - d01 d21) / denom, w = (d00 d21 - d01 d20) / denom,
//               denom = d00 d11 - d01 d01 + 1e-10, u = 1 - v - w; dot products summed x, y, z.
//   6 normals   n_v = normalize(sum over the incident faces, ascending, of angle_f(v) normalize(e0 x e1)); a zero sum gives zero.
//               angle = acos(clamp(dot(normalize(a), normalize(b)), -1, 1)) of the two edges leaving the corner.  acos is the one
//               library call here: the host's and the device's may differ in the last bits of a float64.
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

constexpr int kGiBlock = 256;                                // faces per first-level scan block (= the workgroup)

struct GiMesh {
    int32_t V, F;
    const double *verts;                                     // (V,3)
    const int32_t *faces;                                    // (F,3)
    const uint8_t *mask;                                     // (F) or NULL: 0 = the face is left out
};

struct GiVec { double x, y, z; };
D3GA_FHD GiVec gi_sub(GiVec a, GiVec b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
D3GA_FHD GiVec gi_cross(GiVec a, GiVec b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
D3GA_FHD double gi_dot(GiVec a, GiVec b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
D3GA_FHD double gi_norm(GiVec a) { return sqrt(gi_dot(a, a)); }
D3GA_FHD GiVec gi_normalize(GiVec a) {
    const double n = gi_norm(a), d = n > 1e-12 ? n : 1e-12;
    return {a.x / d, a.y / d, a.z / d};
}
D3GA_FHD GiVec gi_vertex(const double *verts, int32_t v) { return {verts[3 * (size_t)v], verts[3 * (size_t)v + 1], verts[3 * (size_t)v + 2]}; }

D3GA_FHD bool gi_face_in_range(const GiMesh &m, int f) {
    const int32_t *t = m.faces + 3 * (size_t)f;
    return (uint32_t)t[0] < (uint32_t)m.V && (uint32_t)t[1] < (uint32_t)m.V && (uint32_t)t[2] < (uint32_t)m.V;
}

// rule 1: the area of face f (>= 0, finite); *bad is set for a face that names a vertex outside [0, V) -- nothing is read for it
D3GA_FHD double gi_area(const GiMesh &m, int f, bool *bad) {
    if (!gi_face_in_range(m, f)) { *bad = true; return 0.0; }
    if (m.mask && !m.mask[f]) return 0.0;
    const int32_t *t = m.faces + 3 * (size_t)f;
    const GiVec v0 = gi_vertex(m.verts, t[0]);
    const double a = 0.5 * gi_norm(gi_cross(gi_sub(gi_vertex(m.verts, t[1]), v0), gi_sub(gi_vertex(m.verts, t[2]), v0)));
    return a <= 1.7976931348623157e308 ? a : 0.0;            // NaN and infinity weigh nothing
}

D3GA_FHD uint64_t gi_bits(double a) {
    union { double d; uint64_t u; } c;
    c.d = a;
    return c.u;
}

// E with a < 2^E for the non-negative finite double of these bits (a subnormal counts as 2^-1022)
D3GA_FHD int gi_exponent(uint64_t bits) {
    const int be = (int)(bits >> 52) & 0x7ff;
    return be == 0 ? -1022 : be - 1022;
}
D3GA_FHD int gi_ceil_log2(int F) {
    int c = 0;
    while (((int64_t)1 << c) < F) ++c;
    return c;
}
D3GA_FHD int gi_shift(uint64_t max_bits, int F) { return 62 - gi_exponent(max_bits) - gi_ceil_log2(F); }

// floor(a 2^k) of a non-negative finite double as an integer shift of its mantissa; a 2^k < 2^62 by the choice of k
D3GA_FHD uint64_t gi_quantize(double a, int k) {
    const uint64_t bits = gi_bits(a);
    const int be = (int)(bits >> 52) & 0x7ff;
    const uint64_t frac = bits & (((uint64_t)1 << 52) - 1);
    const uint64_t mant = be == 0 ? frac : frac | ((uint64_t)1 << 52);
    const int s = (be == 0 ? -1074 : be - 1075) + k;         // a = mant 2^(s - k)
    if (s >= 0) return s > 9 ? 0 : mant << s;                // s > 9 cannot happen below 2^62; never shift out of the word
    return s <= -64 ? 0 : mant >> (-s);
}

D3GA_FHD uint64_t gi_cum(const uint64_t *cum_local, const uint64_t *block_start, int i) { return block_start[i / kGiBlock] + cum_local[i]; }

// rule 2
D3GA_FHD uint64_t gi_mantissa(double u0) {
    if (!(u0 > 0.0)) return 0;
    const double s = u0 * 9007199254740992.0;                // 2^53: exact
    return s >= 9007199254740991.0 ? 9007199254740991ull : (uint64_t)s;
}
D3GA_FHD uint64_t gi_pick(uint64_t m, uint64_t total) {
#ifdef __HIP_DEVICE_COMPILE__
    return (__umul64hi(m, total) << 11) | ((m * total) >> 53);
#else
    return (uint64_t)(((unsigned __int128)m * total) >> 53);
#endif
}
// the first i with cum[i] > pick; pick < total = cum[F-1]
D3GA_FHD int gi_search(const uint64_t *cum_local, const uint64_t *block_start, int F, uint64_t pick) {
    int lo = 0, hi = F - 1;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (gi_cum(cum_local, block_start, mid) > pick) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

struct GiSample {
    float point[3], quat[4], bary[3];
    int32_t face[3], face_id;
};

// pytorch3d's matrix_to_quaternion on the matrix with columns T, B, N (m_rc: row r, column c), in float64
D3GA_FHD void gi_quaternion(GiVec T, GiVec B, GiVec N, double q[4]) {
    const double m00 = T.x, m01 = B.x, m02 = N.x, m10 = T.y, m11 = B.y, m12 = N.y, m20 = T.z, m21 = B.z, m22 = N.z;
    double s[4] = {1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22, 1.0 - m00 - m11 + m22};
    double a[4];
    int best = 0;
    for (int i = 0; i < 4; ++i) {
        a[i] = s[i] > 0.0 ? sqrt(s[i]) : 0.0;
        if (a[i] > a[best]) best = i;                        // argmax, ties to the first
    }
    const double sq = a[best] * a[best];
    double c[4];
    if (best == 0) { c[0] = sq; c[1] = m21 - m12; c[2] = m02 - m20; c[3] = m10 - m01; }
    else if (best == 1) { c[0] = m21 - m12; c[1] = sq; c[2] = m10 + m01; c[3] = m02 + m20; }
    else if (best == 2) { c[0] = m02 - m20; c[1] = m10 + m01; c[2] = sq; c[3] = m12 + m21; }
    else { c[0] = m10 - m01; c[1] = m20 + m02; c[2] = m21 + m12; c[3] = sq; }
    const double d = 2.0 * (a[best] > 0.1 ? a[best] : 0.1);
    const bool neg = c[0] / d < 0.0;
    for (int i = 0; i < 4; ++i) q[i] = neg ? -(c[i] / d) : c[i] / d;
}

// rules 2 - 5 for one sample; total > 0
D3GA_FHD GiSample gi_sample(const GiMesh &m, const uint64_t *cum_local, const uint64_t *block_start, uint64_t total, const double *u) {
    GiSample o;
    const int f = gi_search(cum_local, block_start, m.F, gi_pick(gi_mantissa(u[0]), total));
    const int32_t *t = m.faces + 3 * (size_t)f;
    o.face_id = f;
    o.face[0] = t[0]; o.face[1] = t[1]; o.face[2] = t[2];
    const GiVec v0 = gi_vertex(m.verts, t[0]);
    const GiVec e0 = gi_sub(gi_vertex(m.verts, t[1]), v0), e1 = gi_sub(gi_vertex(m.verts, t[2]), v0);
    double r1 = u[1], r2 = u[2];
    if (r1 + r2 > 1.0) { r1 = fabs(r1 - 1.0); r2 = fabs(r2 - 1.0); }
    o.point[0] = (float)(v0.x + r1 * e0.x + r2 * e1.x);
    o.point[1] = (float)(v0.y + r1 * e0.y + r2 * e1.y);
    o.point[2] = (float)(v0.z + r1 * e0.z + r2 * e1.z);
    const GiVec N = gi_normalize(gi_cross(e0, e1)), T = gi_normalize(gi_cross(e0, N)), B = gi_normalize(gi_cross(e0, T));
    double q[4];
    gi_quaternion(T, B, N, q);
    for (int i = 0; i < 4; ++i) o.quat[i] = (float)q[i];
    const GiVec p = {(double)o.point[0], (double)o.point[1], (double)o.point[2]};
    const GiVec v2 = gi_sub(p, v0);
    const double d00 = gi_dot(e0, e0), d01 = gi_dot(e0, e1), d11 = gi_dot(e1, e1), d20 = gi_dot(v2, e0), d21 = gi_dot(v2, e1);
    const double denom = (d00 * d11 - d01 * d01) + 0.0000000001;
    const double bv = (d11 * d20 - d01 * d21) / denom, bw = (d00 * d21 - d01 * d20) / denom;
    o.bary[0] = (float)(1.0 - bv - bw);
    o.bary[1] = (float)bv;
    o.bary[2] = (float)bw;
    return o;
}

// rule 6: vertex v over its incident faces csr_faces[csr_offsets[v] .. csr_offsets[v+1]) in list order (ascending)
D3GA_FHD GiVec gi_vertex_normal(const GiMesh &m, const int32_t *csr_offsets, const int32_t *csr_faces, int v, bool *bad) {
    GiVec acc = {0.0, 0.0, 0.0};
    for (int32_t j = csr_offsets[v]; j < csr_offsets[v + 1]; ++j) {
        const int32_t f = csr_faces[j];
        if ((uint32_t)f >= (uint32_t)m.F || !gi_face_in_range(m, f)) { *bad = true; continue; }
        const int32_t *t = m.faces + 3 * (size_t)f;
        const int c = t[0] == v ? 0 : (t[1] == v ? 1 : 2);
        if (t[c] != v) { *bad = true; continue; }            // the list names a face that does not touch v
        const GiVec p0 = gi_vertex(m.verts, t[0]), p1 = gi_vertex(m.verts, t[1]), p2 = gi_vertex(m.verts, t[2]);
        const GiVec n = gi_normalize(gi_cross(gi_sub(p1, p0), gi_sub(p2, p0)));
        const GiVec pc = c == 0 ? p0 : (c == 1 ? p1 : p2), pa = c == 0 ? p1 : (c == 1 ? p2 : p0), pb = c == 0 ? p2 : (c == 1 ? p0 : p1);
        double cosine = gi_dot(gi_normalize(gi_sub(pa, pc)), gi_normalize(gi_sub(pb, pc)));
        cosine = cosine > 1.0 ? 1.0 : (cosine < -1.0 ? -1.0 : cosine);
        const double angle = cosine == cosine ? acos(cosine) : 0.0;
        acc.x += angle * n.x; acc.y += angle * n.y; acc.z += angle * n.z;
    }
    return gi_normalize(acc);
}

// ---- scratch layout and the argument rules of the entry points (include/d3ga.h); nothing is dereferenced --------------------------
//   [0]  header, 256 bytes: word 0 (uint64) the bits of the largest area
//   [1]  cum_local  F uint64
//   [2]  block_total  nblk uint64
//   [3]  block_start  nblk + 1 uint64
static inline int64_t gi_align256(int64_t x) { return (x + 255) & ~int64_t(255); }
static inline int64_t gi_blocks(int64_t F) { return (F + kGiBlock - 1) / kGiBlock; }
static inline int64_t gi_scratch_bytes(int64_t F) { return 256 + gi_align256(8 * F) + gi_align256(8 * gi_blocks(F)) + gi_align256(8 * (gi_blocks(F) + 1)); }

struct GiScratch {
    uint64_t *max_bits, *cum_local, *block_total, *block_start;
};
static inline GiScratch gi_carve(void *base, int64_t F) {
    char *p = static_cast<char *>(base);
    GiScratch s;
    s.max_bits = reinterpret_cast<uint64_t *>(p);    p += 256;
    s.cum_local = reinterpret_cast<uint64_t *>(p);   p += gi_align256(8 * F);
    s.block_total = reinterpret_cast<uint64_t *>(p); p += gi_align256(8 * gi_blocks(F));
    s.block_start = reinterpret_cast<uint64_t *>(p);
    return s;
}

static inline int gi_check_sizes(int32_t V, int32_t F) {
    if (V <= 0 || F <= 0 || F >= D3GA_SAMPLE_MAX_FACES || (int64_t)V * 3 > INT32_MAX) return D3GA_E_SIZE;
    return 0;
}

static inline int gi_check_sample(int32_t V, int32_t F, int32_t n, const double *verts, const int32_t *faces, const uint8_t *mask,
                                  const double *uniforms, float *points, float *rotations, int32_t *out_faces, int32_t *face_id, float *barys,
                                  void *scratch, int64_t scratch_bytes, uint32_t *status, int32_t block) {
    (void)mask;                                              // optional
    if (gi_check_sizes(V, F) != 0 || n <= 0 || (int64_t)n * 4 > INT32_MAX) return D3GA_E_SIZE;
    if (block != 0 && block != 64 && block != 128 && block != 256 && block != 512 && block != 1024) return D3GA_E_CONFIG;
    if (!verts || !faces || !uniforms || !points || !rotations || !out_faces || !face_id || !barys || !scratch || !status) return D3GA_E_NULL;
    if (((uintptr_t)verts | (uintptr_t)uniforms) & 7) return D3GA_E_CONFIG;
    if (((uintptr_t)faces | (uintptr_t)points | (uintptr_t)rotations | (uintptr_t)out_faces | (uintptr_t)face_id | (uintptr_t)barys |
         (uintptr_t)status) & 3) return D3GA_E_CONFIG;
    if ((uintptr_t)scratch & 255) return D3GA_E_CONFIG;
    if (scratch_bytes < gi_scratch_bytes(F)) return D3GA_E_CAPACITY;
    return 0;
}

static inline int gi_check_normals(int32_t V, int32_t F, const double *verts, const int32_t *faces, const int32_t *csr_offsets,
                                   const int32_t *csr_faces, double amount, double *normals, double *inflated, uint32_t *status) {
    if (gi_check_sizes(V, F) != 0) return D3GA_E_SIZE;
    if (!(amount == amount) || amount - amount != 0.0) return D3GA_E_CONFIG;     // NaN or infinite
    if (!verts || !faces || !csr_offsets || !csr_faces || !status || (!normals && !inflated)) return D3GA_E_NULL;
    if (((uintptr_t)verts | (uintptr_t)normals | (uintptr_t)inflated) & 7) return D3GA_E_CONFIG;
    if (((uintptr_t)faces | (uintptr_t)csr_offsets | (uintptr_t)csr_faces | (uintptr_t)status) & 3) return D3GA_E_CONFIG;
    if (inflated == verts || normals == verts) return D3GA_E_CONFIG;             // every vertex reads its neighbours' input positions
    return 0;
}

}  // namespace d3ga
