// mesh_raster_math.h -- the per-element arithmetic of the triangle-mesh rasterizer (mesh_raster.hip): the camera, the face
// record and its two drop rules, screen barycentrics and coverage, perspective-correct depth, the depth key, the flat shader of
// the reference's recorder/mesh_renderer.py:55-67 (pytorch3d's HardFlatShader with the light at the camera centre) and the maps
// of :69-100.  Semantics: DESIGN.md 4.4f (specification of record).  Compiles for the host as it is
// (tests/hostcheck/meshcheck.cpp runs this very text on the CPU against tests/mesh_ref.py); mesh_raster.hip is compiled with
// -ffp-contract=off and correctly rounded division and square root, so the device evaluates every expression here as g++ does.
#pragma once
#include <math.h>
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

constexpr int kMeshChunk = 32;                  // pixels per side of a chunk: the unit of work of one wavefront
constexpr int kMeshMaxSide = D3GA_MESH_MAX_SIDE;
constexpr int kMeshCam = D3GA_MESH_CAM_FLOATS;  // R row-major (9), t (3), fx, fy, cx, cy
constexpr float kMeshNear = 0.01f;              // a face with a vertex at z <= this is dropped
constexpr float kMeshMinArea = 1e-8f;           // ... and one whose doubled screen area is smaller in magnitude, px^2
constexpr uint64_t kMeshEmptyKey = ~(uint64_t)0;

// What coverage and resolve need of a face: 48 bytes.
struct alignas(16) MeshFaceRec {
    float x0, y0, x1, y1;                       // screen positions, pixels
    float x2, y2, area, iz0;                    // doubled signed area; 1 / z_i
    float iz1, iz2;
    int32_t bx, by;                             // first | last << 16 column / row whose pixel centre lies inside the bounding box
};

// view space: R x + t
D3GA_FHD void mesh_view(const float *cam, const float *x, float *v) {
    v[0] = ((cam[0] * x[0] + cam[1] * x[1]) + cam[2] * x[2]) + cam[9];
    v[1] = ((cam[3] * x[0] + cam[4] * x[1]) + cam[5] * x[2]) + cam[10];
    v[2] = ((cam[6] * x[0] + cam[7] * x[1]) + cam[8] * x[2]) + cam[11];
}

// the camera centre -R^T t
D3GA_FHD void mesh_camera_centre(const float *cam, float *c) {
    c[0] = -((cam[0] * cam[9] + cam[3] * cam[10]) + cam[6] * cam[11]);
    c[1] = -((cam[1] * cam[9] + cam[4] * cam[10]) + cam[7] * cam[11]);
    c[2] = -((cam[2] * cam[9] + cam[5] * cam[10]) + cam[8] * cam[11]);
}

// cross(p - a, b - a).  For fixed a, b it is monotone in px at fixed py and in py at fixed px EVEN AS ROUNDED (every operation
// is monotone in its varying operand), so over a rectangle of pixels its extremes sit at the corners: the chunk rejection
// of the coverage kernel loses nothing.
D3GA_FHD float mesh_edge(float px, float py, float ax, float ay, float bx, float by) {
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax);
}

D3GA_FHD int mesh_clamp_index(float v, int hi) {
    v = fmaxf(v, -1.f);                         // NaN -> -1
    v = fminf(v, (float)(hi + 1));
    return (int)v;
}

// The face record of view-space-transformed vertices.  -> the number of chunks its box spans, 0: dropped (a vertex at
// z <= 0.01, |area| < 1e-8, anything not finite, or no pixel centre inside the box).
D3GA_FHD int mesh_face_setup(const float *cam, const float *w0, const float *w1, const float *w2, int H, int W, MeshFaceRec *r) {
    float v0[3], v1[3], v2[3];
    mesh_view(cam, w0, v0);
    mesh_view(cam, w1, v1);
    mesh_view(cam, w2, v2);
    if (!(v0[2] > kMeshNear && v1[2] > kMeshNear && v2[2] > kMeshNear)) return 0;
    const float fx = cam[12], fy = cam[13], cx = cam[14], cy = cam[15];
    r->x0 = fx * v0[0] / v0[2] + cx; r->y0 = fy * v0[1] / v0[2] + cy;
    r->x1 = fx * v1[0] / v1[2] + cx; r->y1 = fy * v1[1] / v1[2] + cy;
    r->x2 = fx * v2[0] / v2[2] + cx; r->y2 = fy * v2[1] / v2[2] + cy;
    r->area = mesh_edge(r->x2, r->y2, r->x0, r->y0, r->x1, r->y1);
    if (!(fabsf(r->area) >= kMeshMinArea) || !(fabsf(r->area) <= 3.0e38f)) return 0;
    r->iz0 = 1.f / v0[2]; r->iz1 = 1.f / v1[2]; r->iz2 = 1.f / v2[2];
    // pixel i samples i + 0.5: the columns with min - 0.5 <= i <= max - 0.5 (the subtraction is exact wherever it matters)
    const float xmin = fminf(r->x0, fminf(r->x1, r->x2)), xmax = fmaxf(r->x0, fmaxf(r->x1, r->x2));
    const float ymin = fminf(r->y0, fminf(r->y1, r->y2)), ymax = fmaxf(r->y0, fmaxf(r->y1, r->y2));
    int i0 = mesh_clamp_index(ceilf(xmin - 0.5f), W), i1 = mesh_clamp_index(floorf(xmax - 0.5f), W);
    int j0 = mesh_clamp_index(ceilf(ymin - 0.5f), H), j1 = mesh_clamp_index(floorf(ymax - 0.5f), H);
    if (i0 < 0) i0 = 0;
    if (j0 < 0) j0 = 0;
    if (i1 > W - 1) i1 = W - 1;
    if (j1 > H - 1) j1 = H - 1;
    if (i0 > i1 || j0 > j1) return 0;
    r->bx = i0 | (i1 << 16);
    r->by = j0 | (j1 << 16);
    return (((i1 - i0) / kMeshChunk) + 1) * (((j1 - j0) / kMeshChunk) + 1);
}

// pytorch3d's interpolate_face_attributes (recorder/mesh_renderer.py:80-93) for one channel of one pixel: the weights are
// taken as they come (the reference passes ones for its normal map), the sum runs in the order b0 a0, b1 a1, b2 a2
D3GA_FHD float mesh_interp_attr(float b0, float b1, float b2, float a0, float a1, float a2) { return (b0 * a0 + b1 * a1) + b2 * a2; }

D3GA_FHD int mesh_box_lo(int32_t packed) { return packed & 0xffff; }
D3GA_FHD int mesh_box_hi(int32_t packed) { return (packed >> 16) & 0xffff; }

// screen barycentrics at a point: edge functions over the signed area
D3GA_FHD void mesh_bary(const MeshFaceRec &r, float px, float py, float *b) {
    b[0] = mesh_edge(px, py, r.x1, r.y1, r.x2, r.y2) / r.area;
    b[1] = mesh_edge(px, py, r.x2, r.y2, r.x0, r.y0) / r.area;
    b[2] = mesh_edge(px, py, r.x0, r.y0, r.x1, r.y1) / r.area;
}

D3GA_FHD bool mesh_inside(const float *b) { return b[0] >= 0.f && b[1] >= 0.f && b[2] >= 0.f; }

// zbuf = 1 / sum b_i / z_i and, with bp, the perspective-correct barycentrics (b_i / z_i) zbuf
D3GA_FHD float mesh_depth(const MeshFaceRec &r, const float *b, float *bp) {
    const float u0 = b[0] * r.iz0, u1 = b[1] * r.iz1, u2 = b[2] * r.iz2;
    const float zbuf = 1.f / ((u0 + u1) + u2);
    if (bp) {
        bp[0] = u0 * zbuf; bp[1] = u1 * zbuf; bp[2] = u2 * zbuf;
    }
    return zbuf;
}

D3GA_FHD uint32_t mesh_float_bits(float v) {
    uint32_t u;
    __builtin_memcpy(&u, &v, 4);
    return u;
}

// Does the face cover pixel (i, j)?  key = float_bits(zbuf) << 32 | face: zbuf > 0, so the smallest key is the nearest face
// and, among equal depths, the smallest face index.
D3GA_FHD bool mesh_cover(const MeshFaceRec &r, int i, int j, uint32_t face, uint64_t *key) {
    float b[3];
    mesh_bary(r, (float)i + 0.5f, (float)j + 0.5f, b);
    if (!mesh_inside(b)) return false;
    const float z = mesh_depth(r, b, nullptr);
    if (!(z > 0.f) || !(z <= 3.0e38f)) return false;
    *key = ((uint64_t)mesh_float_bits(z) << 32) | face;
    return true;
}

// The pixel rectangle of chunk `chunk` of a face's box (chunks are counted row by row from the box's first pixel).
D3GA_FHD void mesh_chunk_rect(const MeshFaceRec &r, uint32_t chunk, int *i0, int *j0, int *i1, int *j1) {
    const int bi0 = mesh_box_lo(r.bx), bi1 = mesh_box_hi(r.bx), bj0 = mesh_box_lo(r.by), bj1 = mesh_box_hi(r.by);
    const uint32_t ncx = (uint32_t)((bi1 - bi0) / kMeshChunk) + 1;
    const int cy = (int)(chunk / ncx), cx = (int)(chunk - (uint32_t)cy * ncx);
    *i0 = bi0 + cx * kMeshChunk;
    *j0 = bj0 + cy * kMeshChunk;
    *i1 = *i0 + kMeshChunk - 1 < bi1 ? *i0 + kMeshChunk - 1 : bi1;
    *j1 = *j0 + kMeshChunk - 1 < bj1 ? *j0 + kMeshChunk - 1 : bj1;
}

// Is some barycentric negative at all four corners (hence at every pixel) of the pixel rectangle [i0, i1] x [j0, j1]?
D3GA_FHD bool mesh_rect_outside(const MeshFaceRec &r, int i0, int j0, int i1, int j1) {
    float a[3], b[3], c[3], d[3];
    mesh_bary(r, (float)i0 + 0.5f, (float)j0 + 0.5f, a);
    mesh_bary(r, (float)i1 + 0.5f, (float)j0 + 0.5f, b);
    mesh_bary(r, (float)i0 + 0.5f, (float)j1 + 0.5f, c);
    mesh_bary(r, (float)i1 + 0.5f, (float)j1 + 0.5f, d);
    bool out = false;
    for (int k = 0; k < 3; ++k) out = out || (!(a[k] >= 0.f) && !(b[k] >= 0.f) && !(c[k] >= 0.f) && !(d[k] >= 0.f));
    return out;
}

// How a wavefront's 64 lanes tile a chunk that is `w` pixels wide: 2^shift lanes along a row (8, 16 or 32: the narrowest that
// holds the row), 64 >> shift rows per step.  Lanes of one row write neighbouring depth keys, which is what the atomic unit wants.
D3GA_FHD int mesh_row_shift(int w) { return w <= 8 ? 3 : (w <= 16 ? 4 : 5); }

D3GA_FHD void mesh_cross_edges(const float *x0, const float *x1, const float *x2, float *n) {
    const float ax = x1[0] - x0[0], ay = x1[1] - x0[1], az = x1[2] - x0[2];
    const float bx = x2[0] - x0[0], by = x2[1] - x0[1], bz = x2[2] - x0[2];
    n[0] = ay * bz - az * by;
    n[1] = az * bx - ax * bz;
    n[2] = ax * by - ay * bx;
}

D3GA_FHD void mesh_normalize(float *v, float eps) {
    const float len = fmaxf(sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]), eps);
    v[0] = v[0] / len; v[1] = v[1] / len; v[2] = v[2] / len;
}

D3GA_FHD float mesh_dot(const float *a, const float *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

D3GA_FHD void mesh_interp(const float *bp, const float *a0, const float *a1, const float *a2, float *out) {
    for (int c = 0; c < 3; ++c) out[c] = (bp[0] * a0[c] + bp[1] * a1[c]) + bp[2] * a2[c];
}

// HardFlatShader with one point light at the camera centre: ambient 0.45, diffuse 0.35, specular 0.05, shininess 64, material
// colours 1.  c0..c2: the vertex colours (all null: ones).
D3GA_FHD void mesh_shade_flat(const float *cam, const float *x0, const float *x1, const float *x2, const float *c0, const float *c1,
                              const float *c2, const float *bp, float *rgb) {
    const float one[3] = {1.f, 1.f, 1.f};
    float texel[3], p[3], n[3], c[3], l[3], rr[3];
    mesh_interp(bp, c0 ? c0 : one, c0 ? c1 : one, c0 ? c2 : one, texel);
    mesh_interp(bp, x0, x1, x2, p);
    mesh_cross_edges(x0, x1, x2, n);
    mesh_normalize(n, 1e-6f);
    mesh_camera_centre(cam, c);
    for (int k = 0; k < 3; ++k) l[k] = c[k] - p[k];
    mesh_normalize(l, 1e-6f);
    const float cosang = mesh_dot(n, l);
    for (int k = 0; k < 3; ++k) rr[k] = 2.f * cosang * n[k] - l[k];
    float s = cosang > 0.f ? fmaxf(mesh_dot(l, rr), 0.f) : 0.f;      // the view direction equals the light direction
    for (int k = 0; k < 6; ++k) s = s * s;                           // ^64
    const float shade = 0.45f + 0.35f * fmaxf(cosang, 0.f);
    for (int k = 0; k < 3; ++k) rgb[k] = shade * texel[k] + 0.05f * s;
}

// Renderer.map at a covered pixel: world position, view depth, and the reference's normal (the three vertex normals ADDED, not
// interpolated, then normalised with the norm clamped at 1e-8).
D3GA_FHD void mesh_map_pixel(const float *cam, const float *x0, const float *x1, const float *x2, const float *n0, const float *n1,
                             const float *n2, const float *bp, float *pos, float *nrm, float *depth) {
    mesh_interp(bp, x0, x1, x2, pos);
    float v0[3], v1[3], v2[3];
    mesh_view(cam, x0, v0);
    mesh_view(cam, x1, v1);
    mesh_view(cam, x2, v2);
    *depth = (bp[0] * v0[2] + bp[1] * v1[2]) + bp[2] * v2[2];
    for (int k = 0; k < 3; ++k) nrm[k] = (n0[k] + n1[k]) + n2[k];
    mesh_normalize(nrm, 1e-8f);
}

// pytorch3d's vertex normal: the un-normalised face crosses of the incident faces, added in the order of the list, normalised
// with the norm clamped at 1e-6.  faces: (F,3) indices;  list: the vertex's n incident faces.
D3GA_FHD void mesh_vertex_normal(const float *verts, const int32_t *faces, const int32_t *list, int n, int V, int F, float *out) {
    float acc[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < n; ++k) {
        if ((uint32_t)list[k] >= (uint32_t)F) continue;
        const int32_t *f = faces + 3 * (int64_t)list[k];
        if ((uint32_t)f[0] >= (uint32_t)V || (uint32_t)f[1] >= (uint32_t)V || (uint32_t)f[2] >= (uint32_t)V) continue;
        float c[3];
        mesh_cross_edges(verts + 3 * (int64_t)f[0], verts + 3 * (int64_t)f[1], verts + 3 * (int64_t)f[2], c);
        acc[0] += c[0]; acc[1] += c[1]; acc[2] += c[2];
    }
    mesh_normalize(acc, 1e-6f);
    out[0] = acc[0]; out[1] = acc[1]; out[2] = acc[2];
}

}  // namespace d3ga
