// mesh_raster.hip -- forward-only triangle-mesh rasterizer behind the reference's recorder/mesh_renderer.py::Renderer
// (pytorch3d MeshRasterizer, blur_radius 0, one face per pixel, + HardFlatShader; Renderer.map).  Semantics: DESIGN.md 4.4f;
// per-element arithmetic: mesh_raster_math.h.  Compiled with -ffp-contract=off and correctly rounded division / square root:
// the device evaluates the header as its g++ build does.
//
// d3ga_mesh_rasterize, five launches, no host synchronisation, no float atomics:
//   mesh_clear_kernel     every depth key := all ones (scratch is never assumed clean).
//   mesh_setup_kernel     one lane per (b, face): the 48-byte face record (screen positions, signed area, 1/z, pixel box) and the
//                         number of 32 x 32-pixel chunks its clamped box spans (0: dropped).  The workgroup's 256 counts are
//                         scanned in LDS: the exclusive prefix inside the workgroup and the workgroup's total are stored.
//   mesh_scan_kernel      one workgroup: exclusive 64-bit prefix of the workgroups' totals; its last entry is the chunk total.
//   mesh_coverage_kernel  a grid-stride loop over chunks, the total read from device memory.  One wavefront per chunk: two
//                         ballot searches (64-ary over the workgroup prefixes, then the 256 prefixes of that workgroup) find
//                         the face; a chunk with some barycentric negative at its four corners is skipped (exact: mesh_edge is
//                         monotone as rounded); the lanes tile the chunk row-wise (8, 16 or 32 lanes along a row, so that one
//                         instruction's keys are neighbours: the atomics execute at the memory side in 64-byte requests) and
//                         issue one 64-bit unsigned atomic min of float_bits(zbuf) << 32 | face per covered pixel, unless a
//                         plain load shows that the key cannot win (keys only fall: a stale load only costs a needless atomic).
//   mesh_resolve_kernel   one lane per pixel: the winning face's barycentrics and depth again from its record.
// The shade, map and vertex-normal kernels are per-pixel / per-vertex gathers over these outputs.
#include "d3ga_internal.h"
#include "mesh_raster_math.h"
#include "wave_prims.h"

namespace d3ga {

constexpr int kMeshScanBlock = 1024;
constexpr int kMeshCoverGrid = 2048;            // workgroups of the coverage kernel: 8 per CU, four wavefronts each

struct MeshScratch {
    uint64_t *keys;          // B H W
    MeshFaceRec *recs;       // B F
    uint32_t *local;         // nblk * kBlock: exclusive prefix of the chunk counts inside a setup workgroup
    uint32_t *block_total;   // nblk
    uint64_t *block_start;   // nblk + 1: exclusive prefix of block_total; [nblk] = all chunks
};
static inline int64_t mesh_blocks(int64_t BF) { return (BF + kBlock - 1) / kBlock; }
static inline int64_t mesh_scratch_bytes(int64_t B, int64_t F, int64_t H, int64_t W) {
    const int64_t nblk = mesh_blocks(B * F);
    return align256(8 * B * H * W) + align256((int64_t)sizeof(MeshFaceRec) * B * F) + align256(4 * nblk * kBlock) + align256(4 * nblk) +
           align256(8 * (nblk + 1));
}
static inline MeshScratch carve_mesh(void *base, int64_t B, int64_t F, int64_t H, int64_t W) {
    const int64_t nblk = mesh_blocks(B * F);
    char *p = (char *)base;
    MeshScratch s;
    s.keys = (uint64_t *)p;         p += align256(8 * B * H * W);
    s.recs = (MeshFaceRec *)p;      p += align256((int64_t)sizeof(MeshFaceRec) * B * F);
    s.local = (uint32_t *)p;        p += align256(4 * nblk * kBlock);
    s.block_total = (uint32_t *)p;  p += align256(4 * nblk);
    s.block_start = (uint64_t *)p;
    return s;
}

__global__ __launch_bounds__(kBlock) void mesh_clear_kernel(uint64_t *__restrict__ keys, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) keys[i] = kMeshEmptyKey;
}

__global__ __launch_bounds__(kBlock) void mesh_setup_kernel(int64_t BF, int F, int V, int H, int W, const float *__restrict__ verts,
                                                            const int32_t *__restrict__ faces, const float *__restrict__ cams,
                                                            MeshFaceRec *__restrict__ recs, uint32_t *__restrict__ local,
                                                            uint32_t *__restrict__ block_total) {
    __shared__ uint32_t s_wave[kBlock / 64];
    const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t count = 0;
    if (g < BF) {
        const int64_t b = g / F;
        const int f = (int)(g - b * F);
        const int32_t i0 = faces[3 * (int64_t)f], i1 = faces[3 * (int64_t)f + 1], i2 = faces[3 * (int64_t)f + 2];
        if ((uint32_t)i0 < (uint32_t)V && (uint32_t)i1 < (uint32_t)V && (uint32_t)i2 < (uint32_t)V) {
            const float *vb = verts + 3 * b * V, *cam = cams + kMeshCam * b;
            float c[kMeshCam], x0[3], x1[3], x2[3];
#pragma unroll
            for (int k = 0; k < kMeshCam; ++k) c[k] = cam[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                x0[k] = vb[3 * (int64_t)i0 + k];
                x1[k] = vb[3 * (int64_t)i1 + k];
                x2[k] = vb[3 * (int64_t)i2 + k];
            }
            MeshFaceRec r;
            count = (uint32_t)mesh_face_setup(c, x0, x1, x2, H, W, &r);
            if (count) recs[g] = r;
        }
    }
    uint32_t total;                             // (the padding lanes of the last workgroup store too: local holds nblk * kBlock words)
    local[g] = block_excl_scan_u32<kBlock / 64>(count, s_wave, &total);
    if (threadIdx.x == 0) block_total[blockIdx.x] = total;
}

__global__ __launch_bounds__(kMeshScanBlock) void mesh_scan_kernel(int64_t nblk, const uint32_t *__restrict__ block_total,
                                                                   uint64_t *__restrict__ block_start) {
    __shared__ uint64_t s_wave[kMeshScanBlock / 64];
    scan_block_totals<kMeshScanBlock>(nblk, block_total, block_start, s_wave);
}

__global__ __launch_bounds__(kBlock) void mesh_coverage_kernel(int64_t nblk, int64_t BF, int F, int H, int W, const MeshFaceRec *__restrict__ recs,
                                                               const uint32_t *__restrict__ local,
                                                               const uint64_t *__restrict__ block_start, uint64_t *keys) {
    const int lane = threadIdx.x & 63;
    const uint64_t n_waves = (uint64_t)gridDim.x * (kBlock / 64);
    const uint64_t total = block_start[nblk];
    for (uint64_t c = (uint64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); c < total; c += n_waves) {
        // the last workgroup whose start is <= c: block_start[lo] <= c < block_start[hi] throughout
        int64_t lo = 0, hi = nblk;
        while (hi - lo > 1) {
            const int64_t step = (hi - lo + 63) / 64;
            const int64_t probe = lo + (lane + 1) * step;
            const bool le = probe < hi && block_start[probe] <= c;
            const int k = __popcll(__ballot(le));            // the starts ascend: the lanes that hold are a prefix
            lo += k * step;
            hi = lo + step < hi ? lo + step : hi;
        }
        const uint32_t rem = (uint32_t)(c - block_start[lo]);           // < this workgroup's total <= 2^26
        // the last of its 256 faces whose exclusive prefix is <= rem (a dropped face shares its prefix with its successor)
        const uint4 q = *reinterpret_cast<const uint4 *>(local + lo * kBlock + 4 * lane);
        const int n_le = __popcll(__ballot(q.x <= rem)) + __popcll(__ballot(q.y <= rem)) + __popcll(__ballot(q.z <= rem)) +
                         __popcll(__ballot(q.w <= rem));
        int64_t g = lo * kBlock + n_le - 1;                  // n_le >= 1: the first prefix is 0
        const bool found = g >= 0 && g < BF;                 // always, by construction
        g = found ? g : 0;
        const MeshFaceRec r = recs[g];
        const uint32_t chunk = rem - local[g];
        const int64_t b = g / F;
        const uint32_t face = (uint32_t)(g - b * F);
        int i0, j0, i1, j1;
        mesh_chunk_rect(r, chunk, &i0, &j0, &i1, &j1);
        // no lane leaves the loop body early: the ballots above need all 64 (the record's box lies inside the frame by construction)
        if (found && i0 >= 0 && j0 >= 0 && i0 <= i1 && j0 <= j1 && i1 < W && j1 < H && !mesh_rect_outside(r, i0, j0, i1, j1)) {
            const int w = i1 - i0 + 1, shift = mesh_row_shift(w);
            const int i = i0 + (lane & ((1 << shift) - 1));
            if (i <= i1) {
                uint64_t *kb = keys + b * H * W;
                for (int j = j0 + (lane >> shift); j <= j1; j += 64 >> shift) {
                    uint64_t key;
                    if (mesh_cover(r, i, j, face, &key)) {
                        uint64_t *p = kb + (int64_t)j * W + i;
                        if (key < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                            atomicMin((unsigned long long *)p, (unsigned long long)key);
                    }
                }
            }
        }
    }
}

__global__ __launch_bounds__(kBlock) void mesh_resolve_kernel(int64_t n, int64_t hw, int W, int F, const uint64_t *__restrict__ keys,
                                                              const MeshFaceRec *__restrict__ recs, int32_t *__restrict__ pix_to_face,
                                                              float *__restrict__ zbuf, float *__restrict__ bary) {
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += (int64_t)gridDim.x * kBlock) {
        const uint64_t key = keys[p];
        const uint32_t face = (uint32_t)key;
        int32_t out = -1;
        float z = -1.f, bp[3] = {-1.f, -1.f, -1.f};
        if (key != kMeshEmptyKey && face < (uint32_t)F) {
            const int64_t b = p / hw;
            const int64_t rem = p - b * hw;
            const int j = (int)(rem / W), i = (int)(rem - (int64_t)j * W);
            const MeshFaceRec r = recs[b * F + face];
            float s[3];
            mesh_bary(r, (float)i + 0.5f, (float)j + 0.5f, s);
            z = mesh_depth(r, s, bp);
            out = (int32_t)face;
        }
        pix_to_face[p] = out;
        if (zbuf) zbuf[p] = z;
        if (bary) { bary[3 * p] = bp[0]; bary[3 * p + 1] = bp[1]; bary[3 * p + 2] = bp[2]; }
    }
}

struct MeshBg {
    float v[3];
};

// the three world positions of a face of mesh b; false: an index outside [0, V)
__device__ __forceinline__ bool mesh_load_face(const float *__restrict__ verts, const int32_t *__restrict__ faces, int64_t b, int V, int f,
                                               int32_t *idx, float *x0, float *x1, float *x2) {
    idx[0] = faces[3 * (int64_t)f]; idx[1] = faces[3 * (int64_t)f + 1]; idx[2] = faces[3 * (int64_t)f + 2];
    if ((uint32_t)idx[0] >= (uint32_t)V || (uint32_t)idx[1] >= (uint32_t)V || (uint32_t)idx[2] >= (uint32_t)V) return false;
    const float *vb = verts + 3 * b * V;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        x0[k] = vb[3 * (int64_t)idx[0] + k];
        x1[k] = vb[3 * (int64_t)idx[1] + k];
        x2[k] = vb[3 * (int64_t)idx[2] + k];
    }
    return true;
}

__global__ __launch_bounds__(kBlock) void mesh_shade_kernel(int64_t n, int64_t hw, int V, int F, const float *__restrict__ verts,
                                                            const int32_t *__restrict__ faces, const float *__restrict__ verts_rgb,
                                                            const float *__restrict__ cams, const int32_t *__restrict__ pix_to_face,
                                                            const float *__restrict__ bary, MeshBg bg, float *__restrict__ image) {
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += (int64_t)gridDim.x * kBlock) {
        const int32_t f = pix_to_face[p];
        float rgb[3] = {bg.v[0], bg.v[1], bg.v[2]};
        int32_t idx[3];
        float x0[3], x1[3], x2[3];
        const int64_t b = p / hw;
        if ((uint32_t)f < (uint32_t)F && mesh_load_face(verts, faces, b, V, f, idx, x0, x1, x2)) {
            float c[kMeshCam], bp[3], c0[3], c1[3], c2[3];
#pragma unroll
            for (int k = 0; k < kMeshCam; ++k) c[k] = cams[kMeshCam * b + k];
#pragma unroll
            for (int k = 0; k < 3; ++k) bp[k] = bary[3 * p + k];
            if (verts_rgb) {
                const float *cb = verts_rgb + 3 * b * V;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    c0[k] = cb[3 * (int64_t)idx[0] + k];
                    c1[k] = cb[3 * (int64_t)idx[1] + k];
                    c2[k] = cb[3 * (int64_t)idx[2] + k];
                }
                mesh_shade_flat(c, x0, x1, x2, c0, c1, c2, bp, rgb);
            } else {
                mesh_shade_flat(c, x0, x1, x2, nullptr, nullptr, nullptr, bp, rgb);
            }
        }
        image[3 * p] = rgb[0]; image[3 * p + 1] = rgb[1]; image[3 * p + 2] = rgb[2];
    }
}

__global__ __launch_bounds__(kBlock) void mesh_maps_kernel(int64_t n, int64_t hw, int V, int F, const float *__restrict__ verts,
                                                           const int32_t *__restrict__ faces, const float *__restrict__ normals,
                                                           const float *__restrict__ cams, const int32_t *__restrict__ pix_to_face,
                                                           const float *__restrict__ bary, float *__restrict__ position,
                                                           float *__restrict__ normal, float *__restrict__ depth, float *__restrict__ mask) {
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += (int64_t)gridDim.x * kBlock) {
        const int32_t f = pix_to_face[p];
        float pos[3] = {0.f, 0.f, 0.f}, nrm[3] = {0.f, 0.f, 0.f}, d = 0.f;
        int32_t idx[3];
        float x0[3], x1[3], x2[3];
        const int64_t b = p / hw;
        if ((uint32_t)f < (uint32_t)F && mesh_load_face(verts, faces, b, V, f, idx, x0, x1, x2)) {
            float c[kMeshCam], bp[3], n0[3], n1[3], n2[3];
#pragma unroll
            for (int k = 0; k < kMeshCam; ++k) c[k] = cams[kMeshCam * b + k];
            const float *nb = normals + 3 * b * V;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                bp[k] = bary[3 * p + k];
                n0[k] = nb[3 * (int64_t)idx[0] + k];
                n1[k] = nb[3 * (int64_t)idx[1] + k];
                n2[k] = nb[3 * (int64_t)idx[2] + k];
            }
            mesh_map_pixel(c, x0, x1, x2, n0, n1, n2, bp, pos, nrm, &d);
        }
        if (position) { position[3 * p] = pos[0]; position[3 * p + 1] = pos[1]; position[3 * p + 2] = pos[2]; }
        if (normal) { normal[3 * p] = nrm[0]; normal[3 * p + 1] = nrm[1]; normal[3 * p + 2] = nrm[2]; }
        if (depth) depth[p] = d;
        if (mask) mask[p] = f > 0 ? 1.f : 0.f;
    }
}

__global__ __launch_bounds__(kBlock) void mesh_vertex_normals_kernel(int64_t n, int V, int F, const float *__restrict__ verts,
                                                                     const int32_t *__restrict__ faces,
                                                                     const int32_t *__restrict__ csr_offsets,
                                                                     const int32_t *__restrict__ csr_faces, float *__restrict__ normals) {
    for (int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x; g < n; g += (int64_t)gridDim.x * kBlock) {
        const int64_t b = g / V;
        const int v = (int)(g - b * V);
        const int32_t begin = csr_offsets[v], end = csr_offsets[v + 1], last = csr_offsets[V];
        float out[3];
        const bool ok = begin >= 0 && end >= begin && end <= last;
        mesh_vertex_normal(verts + 3 * b * V, faces, csr_faces + (ok ? begin : 0), ok ? end - begin : 0, V, F, out);
        normals[3 * g] = out[0]; normals[3 * g + 1] = out[1]; normals[3 * g + 2] = out[2];
    }
}

// one lane per (pixel, channel): the channels of a face corner are contiguous, so loads and stores coalesce
__global__ __launch_bounds__(kBlock) void mesh_interp_kernel(int64_t n, int64_t F_total, int D, const int64_t *__restrict__ pix_to_face,
                                                             const float *__restrict__ bary, const float *__restrict__ face_attrs,
                                                             float *__restrict__ out) {
    for (int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x; g < n; g += (int64_t)gridDim.x * kBlock) {
        const int64_t p = g / D;
        const int c = (int)(g - p * D);
        const int64_t f = pix_to_face[p];
        float v = 0.f;
        if (f >= 0 && f < F_total) {
            const float *a = face_attrs + (size_t)f * 3 * D + c;
            v = mesh_interp_attr(bary[3 * p], bary[3 * p + 1], bary[3 * p + 2], a[0], a[D], a[2 * D]);
        }
        out[g] = v;
    }
}

}  // namespace d3ga

using namespace d3ga;

// sizes every entry point shares: 0 ok
static inline int mesh_sizes(int32_t B, int32_t V, int32_t F) {
    if (B < 0 || V < 0 || F < 0) return D3GA_E_SIZE;
    if ((int64_t)B * F >= ((int64_t)1 << 31)) return D3GA_E_SIZE;
    return D3GA_OK;
}
static inline int mesh_frame(int32_t H, int32_t W) { return (H < 1 || W < 1 || H > kMeshMaxSide || W > kMeshMaxSide) ? D3GA_E_SIZE : D3GA_OK; }

extern "C" int d3ga_mesh_raster_scratch_bytes(int32_t B, int32_t V, int32_t F, int32_t H, int32_t W, size_t *bytes) {
    D3GA_TRY(mesh_sizes(B, V, F));
    D3GA_TRY(mesh_frame(H, W));
    if (!bytes) return D3GA_E_NULL;
    *bytes = (size_t)mesh_scratch_bytes(B, F, H, W) + 256;
    return D3GA_OK;
}

extern "C" int d3ga_mesh_rasterize(int32_t B, int32_t V, int32_t F, int32_t H, int32_t W, const float *verts, const int32_t *faces,
                                   const float *cams, void *scratch, int32_t *pix_to_face, float *zbuf, float *bary,
                                   d3ga_stream_t stream) {
    D3GA_TRY(mesh_sizes(B, V, F));
    D3GA_TRY(mesh_frame(H, W));
    if (!scratch || !pix_to_face || !cams || (F > 0 && (!faces || !verts))) return D3GA_E_NULL;
    if (misaligned(verts) || misaligned(faces) || misaligned(cams) || misaligned(scratch, 15) || misaligned(pix_to_face) ||
        misaligned(zbuf) || misaligned(bary))
        return D3GA_E_CONFIG;
    if (B == 0) return D3GA_OK;
    hipStream_t s = (hipStream_t)stream;
    const int64_t hw = (int64_t)H * W, n = hw * B, BF = (int64_t)B * F, nblk = mesh_blocks(BF);
    const MeshScratch sc = carve_mesh(scratch, B, F, H, W);
    hipLaunchKernelGGL(mesh_clear_kernel, dim3(grid_1d(n)), dim3(kBlock), 0, s, sc.keys, n);
    if (BF > 0) {
        hipLaunchKernelGGL(mesh_setup_kernel, dim3((unsigned)nblk), dim3(kBlock), 0, s, BF, F, V, H, W, verts, faces, cams, sc.recs, sc.local,
                           sc.block_total);
        hipLaunchKernelGGL(mesh_scan_kernel, dim3(1), dim3(kMeshScanBlock), 0, s, nblk, sc.block_total, sc.block_start);
        // no more wavefronts than there can be chunks
        const int64_t most = BF * ((W + kMeshChunk - 1) / kMeshChunk) * ((H + kMeshChunk - 1) / kMeshChunk);
        const int64_t wgs = (most + kBlock / 64 - 1) / (kBlock / 64);
        hipLaunchKernelGGL(mesh_coverage_kernel, dim3((unsigned)(wgs > kMeshCoverGrid ? kMeshCoverGrid : wgs)), dim3(kBlock), 0, s, nblk, BF, F, H,
                           W, sc.recs, sc.local, sc.block_start, sc.keys);
    }
    hipLaunchKernelGGL(mesh_resolve_kernel, dim3(grid_1d(n)), dim3(kBlock), 0, s, n, hw, W, F, sc.keys, sc.recs, pix_to_face, zbuf, bary);
    return check_launch(s, 0);
}

extern "C" int d3ga_mesh_shade_flat(int32_t B, int32_t V, int32_t F, int32_t H, int32_t W, const float *verts, const int32_t *faces,
                                    const float *verts_rgb, const float *cams, const int32_t *pix_to_face, const float *bary,
                                    const float *bg, float *image, d3ga_stream_t stream) {
    D3GA_TRY(mesh_sizes(B, V, F));
    D3GA_TRY(mesh_frame(H, W));
    if (!cams || !pix_to_face || !bary || !bg || !image || (F > 0 && (!faces || !verts))) return D3GA_E_NULL;
    if (misaligned(verts) || misaligned(faces) || misaligned(verts_rgb) || misaligned(cams) || misaligned(pix_to_face) ||
        misaligned(bary) || misaligned(image))
        return D3GA_E_CONFIG;
    if (B == 0) return D3GA_OK;
    hipStream_t s = (hipStream_t)stream;
    const int64_t hw = (int64_t)H * W, n = hw * B;
    MeshBg b;
    b.v[0] = bg[0]; b.v[1] = bg[1]; b.v[2] = bg[2];
    hipLaunchKernelGGL(mesh_shade_kernel, dim3(grid_1d(n)), dim3(kBlock), 0, s, n, hw, V, F, verts, faces, verts_rgb, cams, pix_to_face, bary,
                       b, image);
    return check_launch(s, 0);
}

extern "C" int d3ga_mesh_vertex_normals(int32_t B, int32_t V, int32_t F, const float *verts, const int32_t *faces,
                                        const int32_t *csr_offsets, const int32_t *csr_faces, float *normals, d3ga_stream_t stream) {
    D3GA_TRY(mesh_sizes(B, V, F));
    if (V > 0 && (!verts || !csr_offsets || !normals)) return D3GA_E_NULL;
    if (F > 0 && (!faces || !csr_faces)) return D3GA_E_NULL;
    if (misaligned(verts) || misaligned(faces) || misaligned(csr_offsets) || misaligned(csr_faces) || misaligned(normals))
        return D3GA_E_CONFIG;
    const int64_t n = (int64_t)B * V;
    if (n == 0) return D3GA_OK;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mesh_vertex_normals_kernel, dim3(grid_1d(n)), dim3(kBlock), 0, s, n, V, F, verts, faces, csr_offsets, csr_faces,
                       normals);
    return check_launch(s, 0);
}

extern "C" int d3ga_mesh_maps(int32_t B, int32_t V, int32_t F, int32_t H, int32_t W, const float *verts, const int32_t *faces,
                              const float *vertex_normals, const float *cams, const int32_t *pix_to_face, const float *bary,
                              float *position, float *normal, float *depth, float *mask, d3ga_stream_t stream) {
    D3GA_TRY(mesh_sizes(B, V, F));
    D3GA_TRY(mesh_frame(H, W));
    if (!cams || !pix_to_face || !bary || (F > 0 && (!faces || !verts || !vertex_normals))) return D3GA_E_NULL;
    if (!position && !normal && !depth && !mask) return D3GA_E_NULL;
    if (misaligned(verts) || misaligned(faces) || misaligned(vertex_normals) || misaligned(cams) ||
        misaligned(pix_to_face) || misaligned(bary) || misaligned(position) || misaligned(normal) || misaligned(depth) ||
        misaligned(mask))
        return D3GA_E_CONFIG;
    if (B == 0) return D3GA_OK;
    hipStream_t s = (hipStream_t)stream;
    const int64_t hw = (int64_t)H * W, n = hw * B;
    hipLaunchKernelGGL(mesh_maps_kernel, dim3(grid_1d(n)), dim3(kBlock), 0, s, n, hw, V, F, verts, faces, vertex_normals, cams, pix_to_face,
                       bary, position, normal, depth, mask);
    return check_launch(s, 0);
}

extern "C" int d3ga_interp_face_attrs(int64_t n_pix, int64_t F_total, int D, const int64_t *pix_to_face, const float *bary,
                                      const float *face_attrs, float *out, d3ga_stream_t stream) {
    if (n_pix < 0 || F_total < 0 || D < 1 || D > D3GA_INTERP_MAX_D) return D3GA_E_SIZE;
    if (n_pix >= ((int64_t)1 << 40) || F_total >= ((int64_t)1 << 40)) return D3GA_E_SIZE;
    if (n_pix == 0) return D3GA_OK;
    if (!pix_to_face || !bary || !out || (F_total > 0 && !face_attrs)) return D3GA_E_NULL;
    if (misaligned(pix_to_face, 7) || misaligned(bary) || misaligned(face_attrs) || misaligned(out)) return D3GA_E_CONFIG;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = n_pix * D;
    hipLaunchKernelGGL(mesh_interp_kernel, dim3(grid_1d(n)), dim3(kBlock), 0, s, n, F_total, D, pix_to_face, bary, face_attrs, out);
    return check_launch(s, 0);
}
