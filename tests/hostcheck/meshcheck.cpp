// CPU build of d3ga_amd/csrc/mesh_raster_math.h: the loops of mesh_raster.hip (faces -> chunks -> lanes -> pixels, the
// depth-key minimum, resolve, the shade / map / vertex-normal gathers) around the header's own per-element functions.  Same
// arguments as the d3ga_mesh_* entry points (include/d3ga.h), host memory.  Built by tests/test_mesh_render_host.py
// (g++ -ffp-contract=off).
#include <vector>

#include "../../d3ga_amd/csrc/mesh_raster_math.h"

using namespace d3ga;

static bool load_face(const float *verts, const int32_t *faces, int64_t b, int V, int f, const float **x) {
    for (int k = 0; k < 3; ++k) {
        const int32_t i = faces[3 * (int64_t)f + k];
        if ((uint32_t)i >= (uint32_t)V) return false;
        x[k] = verts + 3 * (b * V + i);
    }
    return true;
}

extern "C" {

// -> the number of atomic-min candidates (covered (pixel, face) pairs) or < 0
int64_t hc_mesh_rasterize(int B, int V, int F, int H, int W, const float *verts, const int32_t *faces, const float *cams,
                          int32_t *pix_to_face, float *zbuf, float *bary) {
    int64_t fragments = 0;
    std::vector<uint64_t> keys((size_t)H * W);
    std::vector<MeshFaceRec> recs(F > 0 ? F : 1);
    for (int64_t b = 0; b < B; ++b) {
        const float *cam = cams + kMeshCam * b;
        for (auto &k : keys) k = kMeshEmptyKey;
        for (int f = 0; f < F; ++f) {
            const float *x[3];
            if (!load_face(verts, faces, b, V, f, x)) continue;
            MeshFaceRec &r = recs[f];
            const int chunks = mesh_face_setup(cam, x[0], x[1], x[2], H, W, &r);
            if (!chunks) continue;
            for (int chunk = 0; chunk < chunks; ++chunk) {
                int i0, j0, i1, j1;
                mesh_chunk_rect(r, (uint32_t)chunk, &i0, &j0, &i1, &j1);
                if (i0 > i1 || j0 > j1 || mesh_rect_outside(r, i0, j0, i1, j1)) continue;
                const int shift = mesh_row_shift(i1 - i0 + 1);
                for (int lane = 0; lane < 64; ++lane) {
                    const int i = i0 + (lane & ((1 << shift) - 1));
                    if (i > i1) continue;
                    for (int j = j0 + (lane >> shift); j <= j1; j += 64 >> shift) {
                        uint64_t key;
                        if (!mesh_cover(r, i, j, (uint32_t)f, &key)) continue;
                        ++fragments;
                        uint64_t &k = keys[(size_t)j * W + i];
                        if (key < k) k = key;
                    }
                }
            }
        }
        for (int j = 0; j < H; ++j)
            for (int i = 0; i < W; ++i) {
                const size_t p = ((size_t)b * H + j) * W + i;
                const uint64_t key = keys[(size_t)j * W + i];
                float z = -1.f, bp[3] = {-1.f, -1.f, -1.f};
                int32_t out = -1;
                if (key != kMeshEmptyKey) {
                    float s[3];
                    out = (int32_t)(uint32_t)key;
                    mesh_bary(recs[out], (float)i + 0.5f, (float)j + 0.5f, s);
                    z = mesh_depth(recs[out], s, bp);
                }
                pix_to_face[p] = out;
                if (zbuf) zbuf[p] = z;
                if (bary)
                    for (int k = 0; k < 3; ++k) bary[3 * p + k] = bp[k];
            }
    }
    return fragments;
}

// every pixel of every box through the plain inside test, no chunks: what the chunk rejection must not change
int64_t hc_mesh_covered_pairs_plain(int B, int V, int F, int H, int W, const float *verts, const int32_t *faces, const float *cams) {
    int64_t n = 0;
    for (int64_t b = 0; b < B; ++b)
        for (int f = 0; f < F; ++f) {
            const float *x[3];
            MeshFaceRec r;
            if (!load_face(verts, faces, b, V, f, x) || !mesh_face_setup(cams + kMeshCam * b, x[0], x[1], x[2], H, W, &r)) continue;
            for (int j = mesh_box_lo(r.by); j <= mesh_box_hi(r.by); ++j)
                for (int i = mesh_box_lo(r.bx); i <= mesh_box_hi(r.bx); ++i) {
                    uint64_t key;
                    n += mesh_cover(r, i, j, (uint32_t)f, &key) ? 1 : 0;
                }
        }
    return n;
}

void hc_mesh_shade_flat(int B, int V, int F, int H, int W, const float *verts, const int32_t *faces, const float *verts_rgb,
                        const float *cams, const int32_t *pix_to_face, const float *bary, const float *bg, float *image) {
    for (int64_t b = 0; b < B; ++b)
        for (int64_t q = 0; q < (int64_t)H * W; ++q) {
            const int64_t p = b * H * W + q;
            const int32_t f = pix_to_face[p];
            float rgb[3] = {bg[0], bg[1], bg[2]};
            const float *x[3];
            if ((uint32_t)f < (uint32_t)F && load_face(verts, faces, b, V, f, x)) {
                const float *c[3] = {nullptr, nullptr, nullptr};
                if (verts_rgb)
                    for (int k = 0; k < 3; ++k) c[k] = verts_rgb + (x[k] - verts);
                mesh_shade_flat(cams + kMeshCam * b, x[0], x[1], x[2], c[0], c[1], c[2], bary + 3 * p, rgb);
            }
            for (int k = 0; k < 3; ++k) image[3 * p + k] = rgb[k];
        }
}

void hc_mesh_vertex_normals(int B, int V, int F, const float *verts, const int32_t *faces, const int32_t *csr_offsets,
                            const int32_t *csr_faces, float *normals) {
    for (int64_t b = 0; b < B; ++b)
        for (int v = 0; v < V; ++v)
            mesh_vertex_normal(verts + 3 * b * V, faces, csr_faces + csr_offsets[v], csr_offsets[v + 1] - csr_offsets[v], V, F,
                               normals + 3 * (b * V + v));
}

void hc_mesh_maps(int B, int V, int F, int H, int W, const float *verts, const int32_t *faces, const float *vertex_normals,
                  const float *cams, const int32_t *pix_to_face, const float *bary, float *position, float *normal, float *depth,
                  float *mask) {
    for (int64_t b = 0; b < B; ++b)
        for (int64_t q = 0; q < (int64_t)H * W; ++q) {
            const int64_t p = b * H * W + q;
            const int32_t f = pix_to_face[p];
            float pos[3] = {0.f, 0.f, 0.f}, nrm[3] = {0.f, 0.f, 0.f}, d = 0.f;
            const float *x[3];
            if ((uint32_t)f < (uint32_t)F && load_face(verts, faces, b, V, f, x))
                mesh_map_pixel(cams + kMeshCam * b, x[0], x[1], x[2], vertex_normals + (x[0] - verts), vertex_normals + (x[1] - verts),
                               vertex_normals + (x[2] - verts), bary + 3 * p, pos, nrm, &d);
            for (int k = 0; k < 3; ++k) {
                position[3 * p + k] = pos[k];
                normal[3 * p + k] = nrm[k];
            }
            depth[p] = d;
            mask[p] = f > 0 ? 1.f : 0.f;
        }
}
}
