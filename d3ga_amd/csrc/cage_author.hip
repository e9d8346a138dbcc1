// cage_author.hip -- cage surface authoring: voxelise, fill, isosurface, the two smoothers and the connected parts.
// The rules are the text of cage_author_math.h; this file adds the addressing, the scans and the launches.  Compiled with
// -ffp-contract=off: the g++ build of that header gives these kernels' bits.
//
//   ca_voxelize    a wavefront per triangle (x `slices` workgroup rows for few triangles): the lanes stride over the voxels of the
//                  triangle's box, so a large box never waits behind one lane; integer atomicOr into the bit-packed grid.
//   ca_fill_*      begin: a thread per word.  round: three launches -- a thread per x row, per (x word, z) column along y, per
//                  (x word, y) column along z; every thread owns the words it writes, the launch boundary is the hand-off.
//   ca_iso_*       totals (a thread per lattice point: crossed edges and faces, wave_prims.h block scans), ONE workgroup over the block
//                  totals, vertices (writes every point's first vertex number), faces (reads its neighbours' numbers).
//   ca_normals / ca_improved / ca_uniform / ca_round   a thread per vertex, double-buffered float64 positions; normals are a gather.
//   ca_parts_*     begin, hook (a thread per edge, integer atomicMin on roots), jump (a thread per face).
// No float atomics, no host synchronisation, no wait on another workgroup.  Status words are sticky (atomicOr of vector lanes).
#include "d3ga_internal.h"
#include "cage_author_math.h"
#include "wave_prims.h"

namespace d3ga {

static_assert(kCaBlock == kBlock, "a scan block is a workgroup");
constexpr int kCaTotalsBlock = 256;
constexpr int kCaWaves = kBlock / 64;

__device__ __forceinline__ void ca_raise(uint32_t *status, uint32_t flags) {
    if (flags) atomicOr(status, flags);
}

// ---- voxelise -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void ca_voxelize_kernel(const d3ga_voxel_grid g, const int32_t V, const int32_t F, const double *__restrict__ verts,
                                                             const int32_t *__restrict__ faces, uint32_t *status) {
    const int64_t tri = (int64_t)blockIdx.x * kCaWaves + (threadIdx.x >> 6);
    if (tri >= F) return;
    const CaTriBox b = ca_tri_prepare(g.radius, V, verts, faces + 3 * tri);
    if (b.bad) { if ((threadIdx.x & 63) == 0 && blockIdx.y == 0) atomicOr(status, (uint32_t)D3GA_CAGE_STATUS_RANGE); return; }
    const int64_t cells = (int64_t)b.nx * b.ny * b.nz, stride = 64 * (int64_t)gridDim.y;
    for (int64_t i = (int64_t)blockIdx.y * 64 + (threadIdx.x & 63); i < cells; i += stride) {
        int32_t x, y, z;
        if (!ca_tri_voxel(b, g.radius, i, &x, &y, &z)) continue;
        if ((uint32_t)x >= (uint32_t)g.D || (uint32_t)y >= (uint32_t)g.D || (uint32_t)z >= (uint32_t)g.D) continue;
        unsigned long long *word = reinterpret_cast<unsigned long long *>(g.bits) + ca_word_at(g.D, g.W, x >> 6, y, z);
        const unsigned long long bit = 1ull << (x & 63);
        if (!(*word & bit)) atomicOr(word, bit);              // a stale read costs one more atomic, never a bit
    }
}

// ---- fill -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void ca_fill_begin_kernel(const d3ga_voxel_grid g, uint64_t *__restrict__ outside) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x, n = (int64_t)g.D * g.D * g.W;
    if (i >= n) return;
    const int32_t w = (int32_t)(i % g.W), y = (int32_t)((i / g.W) % g.D), z = (int32_t)(i / ((int64_t)g.W * g.D));
    outside[i] = ca_border_word(g.bits, g.D, g.W, w, y, z);
}

__global__ __launch_bounds__(kBlock) void ca_fill_x_kernel(const d3ga_voxel_grid g, uint64_t *outside, int32_t *changed) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (int64_t)g.D * g.D) return;
    if (ca_sweep_x(g.bits, outside, g.D, g.W, (int32_t)(i % g.D), (int32_t)(i / g.D))) atomicOr(changed, 1);
}

// along_z = 0: a thread per (w, z), the column along y; 1: a thread per (w, y), the column along z
__global__ __launch_bounds__(kBlock) void ca_fill_line_kernel(const d3ga_voxel_grid g, const int along_z, uint64_t *outside, int32_t *changed) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (int64_t)g.W * g.D) return;
    const int32_t w = (int32_t)(i % g.W), other = (int32_t)(i / g.W);
    const int64_t start = along_z ? ca_word_at(g.D, g.W, w, other, 0) : ca_word_at(g.D, g.W, w, 0, other);
    const int64_t stride = along_z ? (int64_t)g.D * g.W : (int64_t)g.W;
    if (ca_sweep_line(g.bits, outside, start, stride, g.D, ca_row_mask(g.D, w))) atomicOr(changed, 1);
}

__global__ __launch_bounds__(kBlock) void ca_fill_finish_kernel(const d3ga_voxel_grid g, const uint64_t *__restrict__ outside, uint64_t *__restrict__ filled) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x, n = (int64_t)g.D * g.D * g.W;
    if (i < n) filled[i] = ~outside[i] & ca_row_mask(g.D, (int32_t)(i % g.W));
}

// ---- isosurface -----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int ca_point_mask(const CaLattice &g, int64_t i, int64_t N, int32_t *px, int32_t *py, int32_t *pz) {
    if (i >= N) return 0;
    *px = (int32_t)(i % g.P); *py = (int32_t)((i / g.P) % g.P); *pz = (int32_t)(i / ((int64_t)g.P * g.P));
    return ca_corner_mask(g, *px, *py, *pz);
}

__global__ __launch_bounds__(kBlock) void ca_iso_totals_kernel(const CaLattice g, const int64_t N, uint32_t *__restrict__ total_v, uint32_t *__restrict__ total_f) {
    __shared__ uint32_t s_v[kCaWaves], s_f[kCaWaves];
    int32_t px = 0, py = 0, pz = 0;
    const int cm = ca_point_mask(g, (int64_t)blockIdx.x * kBlock + threadIdx.x, N, &px, &py, &pz);
    uint32_t tv, tf;
    block_excl_scan_u32<kCaWaves>((uint32_t)ca_popcount7(ca_cross_mask(cm)), s_v, &tv);
    block_excl_scan_u32<kCaWaves>((uint32_t)ca_cell_faces(cm), s_f, &tf);
    if (threadIdx.x == 0) { total_v[blockIdx.x] = tv; total_f[blockIdx.x] = tf; }
}

__global__ __launch_bounds__(kCaTotalsBlock) void ca_iso_starts_kernel(const int64_t nblk, const uint32_t *__restrict__ total_v, const uint32_t *__restrict__ total_f,
                                                                       uint64_t *start_v, uint64_t *start_f, int64_t *counts) {
    __shared__ uint64_t s_wave[kCaTotalsBlock / 64];
    scan_block_totals<kCaTotalsBlock>(nblk, total_v, start_v, s_wave);
    __syncthreads();
    scan_block_totals<kCaTotalsBlock>(nblk, total_f, start_f, s_wave);
    if (threadIdx.x == 0) { counts[0] = (int64_t)start_v[nblk]; counts[1] = (int64_t)start_f[nblk]; }      // lane 0 wrote both
}

__global__ __launch_bounds__(kBlock) void ca_iso_vertices_kernel(const CaLattice g, const int64_t N, const CaIsoMap map, const int64_t n_vertices,
                                                                 const uint64_t *__restrict__ start_v, uint32_t *__restrict__ vstart, float *__restrict__ out) {
    __shared__ uint32_t s_v[kCaWaves];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int32_t p[3] = {0, 0, 0};
    const int cross = ca_cross_mask(ca_point_mask(g, i, N, &p[0], &p[1], &p[2]));
    uint32_t total;
    const uint32_t before = block_excl_scan_u32<kCaWaves>((uint32_t)ca_popcount7(cross), s_v, &total);
    if (i >= N) return;
    int64_t at = (int64_t)start_v[blockIdx.x] + before;
    vstart[i] = (uint32_t)at;
    for (int t = 0; t < 7; ++t) {
        if (!((cross >> t) & 1)) continue;
        if (at < n_vertices)
            for (int c = 0; c < 3; ++c) out[3 * at + c] = ca_iso_coordinate(map, p[c], t, c);
        ++at;
    }
}

__global__ __launch_bounds__(kBlock) void ca_iso_faces_kernel(const CaLattice g, const int64_t N, const int64_t n_faces, const uint64_t *__restrict__ start_f,
                                                              const uint32_t *__restrict__ vstart, int32_t *__restrict__ out) {
    __shared__ uint32_t s_f[kCaWaves];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int32_t px = 0, py = 0, pz = 0;
    const int cm = ca_point_mask(g, i, N, &px, &py, &pz);
    const int nf = ca_cell_faces(cm);
    uint32_t total;
    const uint32_t before = block_excl_scan_u32<kCaWaves>((uint32_t)nf, s_f, &total);
    if (i >= N || nf == 0) return;
    const int64_t at = (int64_t)start_f[blockIdx.x] + before;
    int32_t rows[36];
    const int n = ca_cell_emit(g, vstart, px, py, pz, cm, rows);
    for (int j = 0; j < 3 * n; ++j)
        if (at + j / 3 < n_faces) out[3 * at + j] = rows[j];
}

// ---- smoothing ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void ca_normals_kernel(const GiMesh m, const int32_t *__restrict__ csr_offsets, const int32_t *__restrict__ csr_faces,
                                                            double *__restrict__ normals, uint32_t *status) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= m.V) return;
    uint32_t flags = 0;
    ca_normal(m, csr_offsets, csr_faces, (int32_t)v, normals + 3 * v, &flags);
    ca_raise(status, flags);
}

__global__ __launch_bounds__(kBlock) void ca_improved_kernel(const d3ga_loop_plan p, const double *__restrict__ x, const double *__restrict__ normals,
                                                             const double lbd, double *__restrict__ out, uint32_t *status) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= p.V) return;
    uint32_t flags = 0;
    ca_improved_step(p, x, normals, (int32_t)v, lbd, out + 3 * v, &flags);
    ca_raise(status, flags);
}

__global__ __launch_bounds__(kBlock) void ca_uniform_kernel(const d3ga_loop_plan p, const double *__restrict__ x, const double factor,
                                                            double *__restrict__ out, uint32_t *status) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= p.V) return;
    uint32_t flags = 0;
    ca_uniform_step(p, x, (int32_t)v, factor, out + 3 * v, &flags);
    ca_raise(status, flags);
}

__global__ __launch_bounds__(kBlock) void ca_round_kernel(const int64_t n, const double *__restrict__ x, float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = (float)x[i];
}

// ---- parts ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void ca_parts_begin_kernel(const int32_t F, int32_t *__restrict__ label) {
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (f < F) label[f] = (int32_t)f;
}

__global__ __launch_bounds__(kBlock) void ca_parts_hook_kernel(const d3ga_loop_plan p, int32_t *label, int32_t *changed) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= p.E) return;
    int32_t larger, smaller;
    if (!ca_edge_roots(p, label, (int32_t)e, &larger, &smaller)) return;
    atomicMin(label + larger, smaller);
    atomicOr(changed, 1);
}

__global__ __launch_bounds__(kBlock) void ca_parts_jump_kernel(const int32_t F, int32_t *label) {
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (f < F) label[f] = ca_root(label, (int32_t)f);
}

static inline unsigned ca_grid(int64_t n) { return (unsigned)ca_blocks(n); }

}  // namespace d3ga

using namespace d3ga;

extern "C" int d3ga_cage_voxelize(const d3ga_voxel_grid *grid, int32_t V, int32_t F, const double *verts, const int32_t *faces, uint32_t *status,
                                  d3ga_stream_t stream) {
    D3GA_TRY(ca_check_voxelize(grid, V, F, verts, faces, status));
    hipStream_t s = (hipStream_t)stream;
    D3GA_HIP(zero_async(grid->bits, (size_t)8 * grid->D * grid->D * grid->W, s));
    // few triangles: more lanes per triangle, so that one whose box is the whole grid is shared by up to 256 x 64 lanes
    const int64_t slices = 16384 / F < 1 ? 1 : (16384 / F > 256 ? 256 : 16384 / F);
    hipLaunchKernelGGL(ca_voxelize_kernel, dim3((unsigned)((F + kCaWaves - 1) / kCaWaves), (unsigned)slices), dim3(kBlock), 0, s, *grid, V, F, verts, faces,
                       status);
    return check_launch(s, 0);
}

extern "C" int d3ga_cage_fill(const d3ga_voxel_grid *surface, int32_t stage, uint64_t *outside, uint64_t *filled, int32_t *changed, d3ga_stream_t stream) {
    D3GA_TRY(ca_check_fill(surface, stage, outside, filled, changed));
    hipStream_t s = (hipStream_t)stream;
    const d3ga_voxel_grid g = *surface;
    const int64_t words = (int64_t)g.D * g.D * g.W;
    if (stage == D3GA_CAGE_FILL_BEGIN) {
        hipLaunchKernelGGL(ca_fill_begin_kernel, dim3(ca_grid(words)), dim3(kBlock), 0, s, g, outside);
    } else if (stage == D3GA_CAGE_FILL_ROUND) {
        hipLaunchKernelGGL(ca_fill_x_kernel, dim3(ca_grid((int64_t)g.D * g.D)), dim3(kBlock), 0, s, g, outside, changed);
        hipLaunchKernelGGL(ca_fill_line_kernel, dim3(ca_grid((int64_t)g.W * g.D)), dim3(kBlock), 0, s, g, 0, outside, changed);
        hipLaunchKernelGGL(ca_fill_line_kernel, dim3(ca_grid((int64_t)g.W * g.D)), dim3(kBlock), 0, s, g, 1, outside, changed);
    } else {
        hipLaunchKernelGGL(ca_fill_finish_kernel, dim3(ca_grid(words)), dim3(kBlock), 0, s, g, outside, filled);
    }
    return check_launch(s, 0);
}

extern "C" int d3ga_cage_iso_scratch_bytes(int32_t radius, int64_t *bytes) {
    if (!bytes) return D3GA_E_NULL;
    if (radius < 1 || radius > kCaMaxRadius) return D3GA_E_SIZE;
    *bytes = ca_iso_scratch_bytes(radius);
    return 0;
}

extern "C" int d3ga_cage_iso_count(const d3ga_voxel_grid *grid, void *scratch, int64_t scratch_bytes, int64_t *counts, d3ga_stream_t stream) {
    D3GA_TRY(ca_check_iso_count(grid, scratch, scratch_bytes, counts));
    hipStream_t s = (hipStream_t)stream;
    const CaLattice g = {grid->D, grid->W, grid->D + 1, grid->bits};
    const int64_t N = ca_lattice_points(grid->radius), nb = ca_blocks(N);
    const CaIsoScratch sc = ca_iso_carve(scratch, grid->radius);
    hipLaunchKernelGGL(ca_iso_totals_kernel, dim3((unsigned)nb), dim3(kBlock), 0, s, g, N, sc.total_v, sc.total_f);
    hipLaunchKernelGGL(ca_iso_starts_kernel, dim3(1), dim3(kCaTotalsBlock), 0, s, nb, sc.total_v, sc.total_f, sc.start_v, sc.start_f, counts);
    return check_launch(s, 0);
}

extern "C" int d3ga_cage_iso_emit(const d3ga_voxel_grid *grid, const d3ga_cage_iso_desc *out, void *scratch, int64_t scratch_bytes, d3ga_stream_t stream) {
    D3GA_TRY(ca_check_iso_emit(grid, out, scratch, scratch_bytes));
    hipStream_t s = (hipStream_t)stream;
    const CaLattice g = {grid->D, grid->W, grid->D + 1, grid->bits};
    const int64_t N = ca_lattice_points(grid->radius), nb = ca_blocks(N);
    const CaIsoScratch sc = ca_iso_carve(scratch, grid->radius);
    const CaIsoMap map = {grid->radius, 0, {out->centre[0], out->centre[1], out->centre[2]}, {out->scale[0], out->scale[1], out->scale[2]}};
    hipLaunchKernelGGL(ca_iso_vertices_kernel, dim3((unsigned)nb), dim3(kBlock), 0, s, g, N, map, (int64_t)out->n_vertices, sc.start_v, sc.vstart, out->vertices);
    hipLaunchKernelGGL(ca_iso_faces_kernel, dim3((unsigned)nb), dim3(kBlock), 0, s, g, N, (int64_t)out->n_faces, sc.start_f, sc.vstart, out->faces);
    return check_launch(s, 0);
}

extern "C" int d3ga_cage_smooth(const d3ga_loop_plan *plan, const d3ga_cage_smooth_desc *smooth, d3ga_stream_t stream) {
    D3GA_TRY(ca_check_smooth(plan, smooth));
    hipStream_t s = (hipStream_t)stream;
    const d3ga_cage_smooth_desc d = *smooth;
    const unsigned blocks = ca_grid(plan->V);
    double *cur = d.x, *next = d.work;
    for (int32_t it = 0; it < d.iterations; ++it) {
        if (d.mode == D3GA_CAGE_SMOOTH_IMPROVED) {
            const GiMesh m = {plan->V, plan->F, cur, d.faces, nullptr};
            hipLaunchKernelGGL(ca_normals_kernel, dim3(blocks), dim3(kBlock), 0, s, m, d.csr_offsets, d.csr_faces, d.normals, d.status);
            hipLaunchKernelGGL(ca_improved_kernel, dim3(blocks), dim3(kBlock), 0, s, *plan, cur, d.normals, d.lam, next, d.status);
            double *t = cur; cur = next; next = t;
        } else {
            hipLaunchKernelGGL(ca_uniform_kernel, dim3(blocks), dim3(kBlock), 0, s, *plan, cur, d.lam, next, d.status);
            hipLaunchKernelGGL(ca_uniform_kernel, dim3(blocks), dim3(kBlock), 0, s, *plan, next, d.mu, cur, d.status);
        }
    }
    hipLaunchKernelGGL(ca_round_kernel, dim3(ca_grid(3 * (int64_t)plan->V)), dim3(kBlock), 0, s, 3 * (int64_t)plan->V, cur, d.out);
    return check_launch(s, 0);
}

extern "C" int d3ga_cage_components(const d3ga_loop_plan *plan, int32_t stage, int32_t *label, int32_t *changed, d3ga_stream_t stream) {
    D3GA_TRY(ca_check_components(plan, stage, label, changed));
    hipStream_t s = (hipStream_t)stream;
    if (stage == D3GA_CAGE_PARTS_BEGIN) {
        hipLaunchKernelGGL(ca_parts_begin_kernel, dim3(ca_grid(plan->F)), dim3(kBlock), 0, s, plan->F, label);
    } else {
        hipLaunchKernelGGL(ca_parts_hook_kernel, dim3(ca_grid(plan->E)), dim3(kBlock), 0, s, *plan, label, changed);
        hipLaunchKernelGGL(ca_parts_jump_kernel, dim3(ca_grid(plan->F)), dim3(kBlock), 0, s, plan->F, label);
    }
    return check_launch(s, 0);
}
