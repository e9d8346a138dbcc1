// gauss_init.hip -- Gaussian initialisation: area-weighted surface samples with their frames, quaternions and
// triangle barycentrics, and angle-weighted vertex normals -- the reference's lib/cage.py::CageBase.sample_initial_points between
// a mesh and (points, rotations, faces, barys).  The rules are the text of gauss_init_math.h; this file adds the addressing and
// the scans.  Compiled with -ffp-contract=off: the g++ build of that header gives these kernels' bits.
//
//   gi_clear         zeroes the cell of the largest area (a kernel, not a memset node: d3ga_internal.h).
//   gi_max_area      a thread per face: atomicMax of the area's bit pattern.  Non-negative doubles order as their bits do, so the
//                    maximum is exact whatever the order of arrival.  One atomic per wavefront (the butterfly maximum first).
//   gi_weights       a thread per face, kGiBlock faces per workgroup: q_f = floor(area 2^k), the inclusive 64-bit scan inside the
//                    workgroup (wave_prims.h) and the workgroup's total.  Integers: exact, associative, no floating-point scan.
//   gi_block_starts  ONE workgroup: the exclusive prefix of the workgroup totals (scan_block_totals); block_start[nblk] = total.
//   gi_sample        a thread per sample: binary search over cum = block_start + cum_local, point, frame, quaternion,
//                    barycentrics.  Every output is written once; the quaternion row as one 16-byte store where the base allows.
//   gi_normals       a thread per vertex over MeshTopology's incident-face lists, in list order.
// No float atomics and no host synchronisation.  The status word is sticky (atomicOr of vector lanes).
#include "d3ga_internal.h"
#include "gauss_init_math.h"
#include "wave_prims.h"

namespace d3ga {

static_assert(kGiBlock == kBlock, "a scan block is a workgroup");
constexpr int kGiTotalsBlock = 256;

__global__ void gi_clear_kernel(uint64_t *max_bits) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *max_bits = 0;
}

__global__ __launch_bounds__(kBlock) void gi_max_area_kernel(const GiMesh m, uint64_t *max_bits, uint32_t *status) {
    const int f = blockIdx.x * kBlock + threadIdx.x;
    bool bad = false;
    uint64_t bits = f < m.F ? gi_bits(gi_area(m, f, &bad)) : 0;
    if (bad) atomicOr(status, (uint32_t)D3GA_SAMPLE_STATUS_RANGE);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)bits, off), hi = __shfl_xor((uint32_t)(bits >> 32), off);
        const uint64_t o = ((uint64_t)hi << 32) | lo;
        bits = o > bits ? o : bits;
    }
    if ((threadIdx.x & 63) == 0 && bits != 0) atomicMax((unsigned long long *)max_bits, (unsigned long long)bits);
}

__global__ __launch_bounds__(kBlock) void gi_weights_kernel(const GiMesh m, const uint64_t *__restrict__ max_bits,
                                                            uint64_t *__restrict__ cum_local, uint64_t *__restrict__ block_total) {
    __shared__ uint64_t s_wave[kBlock / 64];
    const int f = blockIdx.x * kBlock + threadIdx.x;
    const int k = gi_shift(*max_bits, m.F);
    bool bad = false;
    const uint64_t q = f < m.F ? gi_quantize(gi_area(m, f, &bad), k) : 0;
    uint64_t total;
    const uint64_t incl = block_incl_scan_u64<kBlock / 64>(q, s_wave, &total);
    if (f < m.F) cum_local[f] = incl;
    if (threadIdx.x == 0) block_total[blockIdx.x] = total;
}

__global__ __launch_bounds__(kGiTotalsBlock) void gi_block_starts_kernel(int64_t nblk, const uint64_t *__restrict__ block_total,
                                                                         uint64_t *__restrict__ block_start) {
    __shared__ uint64_t s_wave[kGiTotalsBlock / 64];
    scan_block_totals<kGiTotalsBlock>(nblk, block_total, block_start, s_wave);
}

struct GiOut {
    float *points, *rotations, *barys;
    int32_t *faces, *face_id;
};

__global__ void gi_sample_kernel(const GiMesh m, const int n, const double *__restrict__ uniforms, const uint64_t *__restrict__ cum_local,
                                 const uint64_t *__restrict__ block_start, const int64_t nblk, const GiOut out, const int rot16,
                                 uint32_t *status) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t total = block_start[nblk];
    GiSample s;
    if (total == 0) {                                        // nothing to sample from: a flag, zeros, face_id -1
        if (i == 0) atomicOr(status, (uint32_t)D3GA_SAMPLE_STATUS_EMPTY);
        s = GiSample{};
        s.face_id = -1;
    } else {
        const double u[3] = {uniforms[3 * (size_t)i], uniforms[3 * (size_t)i + 1], uniforms[3 * (size_t)i + 2]};
        s = gi_sample(m, cum_local, block_start, total, u);
    }
    const size_t r = (size_t)i;
    out.points[3 * r] = s.point[0]; out.points[3 * r + 1] = s.point[1]; out.points[3 * r + 2] = s.point[2];
    if (rot16) reinterpret_cast<float4 *>(out.rotations)[r] = make_float4(s.quat[0], s.quat[1], s.quat[2], s.quat[3]);
    else { out.rotations[4 * r] = s.quat[0]; out.rotations[4 * r + 1] = s.quat[1]; out.rotations[4 * r + 2] = s.quat[2]; out.rotations[4 * r + 3] = s.quat[3]; }
    out.faces[3 * r] = s.face[0]; out.faces[3 * r + 1] = s.face[1]; out.faces[3 * r + 2] = s.face[2];
    out.face_id[r] = s.face_id;
    out.barys[3 * r] = s.bary[0]; out.barys[3 * r + 1] = s.bary[1]; out.barys[3 * r + 2] = s.bary[2];
}

__global__ __launch_bounds__(kBlock) void gi_normals_kernel(const GiMesh m, const int32_t *__restrict__ csr_offsets,
                                                            const int32_t *__restrict__ csr_faces, const double amount,
                                                            double *__restrict__ normals, double *__restrict__ inflated, uint32_t *status) {
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= m.V) return;
    bool bad = false;
    const GiVec nv = gi_vertex_normal(m, csr_offsets, csr_faces, v, &bad);
    if (bad) atomicOr(status, (uint32_t)D3GA_SAMPLE_STATUS_RANGE);
    const size_t r = 3 * (size_t)v;
    if (normals) { normals[r] = nv.x; normals[r + 1] = nv.y; normals[r + 2] = nv.z; }
    if (inflated) {
        inflated[r] = m.verts[r] + amount * nv.x;
        inflated[r + 1] = m.verts[r + 1] + amount * nv.y;
        inflated[r + 2] = m.verts[r + 2] + amount * nv.z;
    }
}

}  // namespace d3ga

using namespace d3ga;

extern "C" int d3ga_surface_sample_scratch_bytes(int32_t F, int64_t *bytes) {
    if (!bytes) return D3GA_E_NULL;
    if (F <= 0 || F >= D3GA_SAMPLE_MAX_FACES) return D3GA_E_SIZE;
    *bytes = gi_scratch_bytes(F);
    return 0;
}

extern "C" int d3ga_surface_sample(int32_t V, int32_t F, int32_t n, const double *verts, const int32_t *faces, const uint8_t *face_mask,
                                   const double *uniforms, float *points, float *rotations, int32_t *out_faces, int32_t *face_id, float *barys,
                                   void *scratch, int64_t scratch_bytes, uint32_t *status, int32_t block, d3ga_stream_t stream) {
    D3GA_TRY(gi_check_sample(V, F, n, verts, faces, face_mask, uniforms, points, rotations, out_faces, face_id, barys, scratch, scratch_bytes,
                             status, block));
    hipStream_t s = (hipStream_t)stream;
    const GiMesh m = {V, F, verts, faces, face_mask};
    const GiScratch sc = gi_carve(scratch, F);
    const int64_t nblk = gi_blocks(F);
    const int lanes = block ? block : kBlock;
    const GiOut out = {points, rotations, barys, out_faces, face_id};
    hipLaunchKernelGGL(gi_clear_kernel, dim3(1), dim3(64), 0, s, sc.max_bits);
    hipLaunchKernelGGL(gi_max_area_kernel, dim3((unsigned)nblk), dim3(kBlock), 0, s, m, sc.max_bits, status);
    hipLaunchKernelGGL(gi_weights_kernel, dim3((unsigned)nblk), dim3(kBlock), 0, s, m, sc.max_bits, sc.cum_local, sc.block_total);
    hipLaunchKernelGGL(gi_block_starts_kernel, dim3(1), dim3(kGiTotalsBlock), 0, s, nblk, sc.block_total, sc.block_start);
    hipLaunchKernelGGL(gi_sample_kernel, dim3((unsigned)(((int64_t)n + lanes - 1) / lanes)), dim3(lanes), 0, s, m, n, uniforms, sc.cum_local,
                       sc.block_start, nblk, out, (int)aligned16(rotations), status);
    return check_launch(s, 0);
}

extern "C" int d3ga_vertex_normals_angle(int32_t V, int32_t F, const double *verts, const int32_t *faces, const int32_t *csr_offsets,
                                         const int32_t *csr_faces, double amount, double *normals, double *inflated, uint32_t *status,
                                         d3ga_stream_t stream) {
    D3GA_TRY(gi_check_normals(V, F, verts, faces, csr_offsets, csr_faces, amount, normals, inflated, status));
    hipStream_t s = (hipStream_t)stream;
    const GiMesh m = {V, F, verts, faces, nullptr};
    hipLaunchKernelGGL(gi_normals_kernel, dim3(grid_1d(V, INT32_MAX)), dim3(kBlock), 0, s, m, csr_offsets, csr_faces, amount, normals, inflated,
                       status);
    return check_launch(s, 0);
}
