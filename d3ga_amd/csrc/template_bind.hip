// template_bind.hip -- template binding: the topology of one level of Loop subdivision built on the device, the
// subdivision stencils over any number of columns, the four-for-one faces, and unpose.  The rules are the text of
// template_bind_math.h; this file adds the addressing, the scans and the counting.  Compiled with -ffp-contract=off: the g++ build of
// that header gives these kernels' bits.
//
//   tb_keys        a thread per face edge: larger << 32 | smaller; the caller sorts (stable) and hands back keys + permutation.
//   tb_heads       a thread per sorted position: 1 where a run of equal keys starts.
//   tb_scan_*      the exclusive prefix of an int32 array in three launches: block totals (wave_prims.h block_excl_scan_u32), ONE
//                  workgroup over the totals (scan_block_totals), the write.  Used for the edge numbers and for the CSR offsets.
//   tb_edges       a thread per sorted position: face edge -> unique edge; a run's head writes the edge's row of every table, counts
//                  the edge at both ends (integer atomicAdd: a count does not depend on the order of arrival) and marks boundary ends.
//   tb_csr_fill    a thread per unique edge: each end takes the next free slot of the other's list (integer cursor) -- in any order --
//   tb_csr_sort    and a thread per vertex sorts its list ascending, so the table no longer knows the order of arrival; the largest
//                  valence by integer atomicMax, one per wavefront.
//   tb_stencil     a thread per output element (row, column) of the (V + E, D) result.
//   tb_faces       a thread per face: its four faces.
//   tb_unpose      a thread per vertex; the (n,4,4) blends live in registers only.
// No float atomics and no host synchronisation.  The status word is sticky (atomicOr of vector lanes).
#include "d3ga_internal.h"
#include "template_bind_math.h"
#include "wave_prims.h"

namespace d3ga {

static_assert(kTbBlock == kBlock, "a scan block is a workgroup");
constexpr int kTbTotalsBlock = 256;

__device__ __forceinline__ void tb_raise(uint32_t *status, uint32_t flags) {
    if (flags) atomicOr(status, flags);
}

__global__ __launch_bounds__(kBlock) void tb_keys_kernel(const int32_t V, const int64_t n, const int32_t *__restrict__ faces,
                                                         int64_t *__restrict__ keys, uint32_t *status) {
    const int64_t h = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (h >= n) return;
    uint32_t flags = 0;
    keys[h] = tb_edge_key(V, faces, h, &flags);
    tb_raise(status, flags);
}

__global__ __launch_bounds__(kBlock) void tb_heads_kernel(const int64_t n, const int64_t *__restrict__ keys, int32_t *__restrict__ head) {
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p < n) head[p] = tb_is_head(keys, p);
}

__global__ __launch_bounds__(kBlock) void tb_scan_totals_kernel(const int64_t n, const int32_t *__restrict__ vals, uint32_t *__restrict__ block_total) {
    __shared__ uint32_t s_wave[kBlock / 64];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t total;
    block_excl_scan_u32<kBlock / 64>(i < n ? (uint32_t)vals[i] : 0u, s_wave, &total);
    if (threadIdx.x == 0) block_total[blockIdx.x] = total;
}

__global__ __launch_bounds__(kTbTotalsBlock) void tb_scan_starts_kernel(const int64_t nblk, const uint32_t *__restrict__ block_total,
                                                                        uint64_t *__restrict__ block_start) {
    __shared__ uint64_t s_wave[kTbTotalsBlock / 64];
    scan_block_totals<kTbTotalsBlock>(nblk, block_total, block_start, s_wave);
}

// excl[i] = sum of vals[0..i); excl[n] = the total
__global__ __launch_bounds__(kBlock) void tb_scan_write_kernel(const int64_t n, const int32_t *__restrict__ vals, const uint64_t *__restrict__ block_start,
                                                               int32_t *__restrict__ excl) {
    __shared__ uint32_t s_wave[kBlock / 64];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t total;
    const uint32_t before = block_excl_scan_u32<kBlock / 64>(i < n ? (uint32_t)vals[i] : 0u, s_wave, &total);
    if (i < n) excl[i] = (int32_t)(block_start[blockIdx.x] + before);
    if (i == n - 1) excl[n] = (int32_t)(block_start[blockIdx.x] + total);
}

__global__ __launch_bounds__(kBlock) void tb_edges_kernel(const d3ga_loop_plan plan, const int64_t n, const int32_t *__restrict__ faces,
                                                          const int64_t *__restrict__ keys, const int64_t *__restrict__ perm,
                                                          const int32_t *__restrict__ head, const int32_t *__restrict__ excl,
                                                          int32_t *__restrict__ valence, int32_t *info) {
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    if (p == 0) info[0] = excl[n];
    const int64_t h = perm[p];
    if ((uint64_t)h >= (uint64_t)n) { atomicOr((uint32_t *)(info + 2), (uint32_t)D3GA_BIND_STATUS_RANGE); return; }
    if (keys[p] == kTbBadKey) { plan.face_edge[h] = -1; return; }
    const int32_t e = head[p] ? excl[p] : excl[p] - 1;       // a member of a run: the run's head came before
    if (e < 0 || (int64_t)e >= n) return;
    plan.face_edge[h] = e;
    if (!head[p]) return;
    uint32_t flags = 0;
    const TbEdge ed = tb_edge_at(plan.V, n, keys, perm, faces, p, &flags);
    tb_raise((uint32_t *)(info + 2), flags);
    plan.edge_verts[2 * (size_t)e] = ed.lo;  plan.edge_verts[2 * (size_t)e + 1] = ed.hi;
    plan.edge_opp[2 * (size_t)e] = ed.o0;    plan.edge_opp[2 * (size_t)e + 1] = ed.o1;
    plan.edge_faces[2 * (size_t)e] = ed.f0;  plan.edge_faces[2 * (size_t)e + 1] = ed.f1;
    plan.edge_boundary[e] = ed.boundary ? 1 : 0;
    if (ed.lo < 0) return;
    atomicAdd(valence + ed.lo, 1);
    atomicAdd(valence + ed.hi, 1);
    if (ed.boundary) { plan.vert_boundary[ed.lo] = 1; plan.vert_boundary[ed.hi] = 1; }      // every writer writes 1
}

__global__ __launch_bounds__(kBlock) void tb_csr_fill_kernel(const d3ga_loop_plan plan, const int32_t *__restrict__ n_edges, int32_t *__restrict__ cursor) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= *n_edges) return;
    const int32_t lo = plan.edge_verts[2 * (size_t)e], hi = plan.edge_verts[2 * (size_t)e + 1];
    if ((uint32_t)lo >= (uint32_t)plan.V || (uint32_t)hi >= (uint32_t)plan.V) return;
    const int32_t a = plan.vert_offsets[lo] + atomicAdd(cursor + lo, 1), b = plan.vert_offsets[hi] + atomicAdd(cursor + hi, 1);
    if (a < plan.vert_offsets[lo + 1]) plan.vert_nbr[a] = hi;
    if (b < plan.vert_offsets[hi + 1]) plan.vert_nbr[b] = lo;
}

__global__ __launch_bounds__(kBlock) void tb_csr_sort_kernel(const d3ga_loop_plan plan, int32_t *info) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int32_t k = 0;
    if (v < plan.V) {
        const int32_t begin = plan.vert_offsets[v], end = plan.vert_offsets[v + 1];
        k = end - begin;
        tb_sort_segment(plan.vert_nbr, begin, end);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) k = max(k, __shfl_xor(k, off));
    if ((threadIdx.x & 63) == 0 && k > 0) atomicMax(info + 1, k);
}

__global__ __launch_bounds__(kBlock) void tb_stencil_kernel(const d3ga_loop_plan plan, const int32_t D, const int64_t total,
                                                            const double *__restrict__ x, const double *__restrict__ beta, const int32_t n_beta,
                                                            float *__restrict__ out, uint32_t *status) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    uint32_t flags = 0;
    out[i] = tb_stencil(plan, x, D, i, beta, n_beta, &flags);
    tb_raise(status, flags);
}

__global__ __launch_bounds__(kBlock) void tb_faces_kernel(const d3ga_loop_plan plan, const int32_t *__restrict__ faces, int32_t *__restrict__ out) {
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (f >= plan.F) return;
    int32_t rows[12];
    tb_face_rows(plan, faces, (int32_t)f, rows);
#pragma unroll
    for (int i = 0; i < 12; ++i) out[12 * (size_t)f + i] = rows[i];
}

template <typename TW>
__global__ __launch_bounds__(kBlock) void tb_unpose_kernel(const TbUnpose u, const TW *__restrict__ skin_w, float *__restrict__ out, uint32_t *status) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= u.n) return;
    uint32_t flags = 0;
    float x[3];
    tb_unpose_one<TW>(u, skin_w, (int32_t)i, x, &flags);
    tb_raise(status, flags);
    out[3 * (size_t)i] = x[0]; out[3 * (size_t)i + 1] = x[1]; out[3 * (size_t)i + 2] = x[2];
}

static int tb_scan(int64_t n, const int32_t *vals, int32_t *excl, const TbScratch &sc, hipStream_t s) {
    const int64_t nblk = tb_blocks(n);
    hipLaunchKernelGGL(tb_scan_totals_kernel, dim3((unsigned)nblk), dim3(kBlock), 0, s, n, vals, sc.block_total);
    hipLaunchKernelGGL(tb_scan_starts_kernel, dim3(1), dim3(kTbTotalsBlock), 0, s, nblk, sc.block_total, sc.block_start);
    hipLaunchKernelGGL(tb_scan_write_kernel, dim3((unsigned)nblk), dim3(kBlock), 0, s, n, vals, sc.block_start, excl);
    return check_launch(s, 0);
}

}  // namespace d3ga

using namespace d3ga;

extern "C" int d3ga_loop_edge_keys(int32_t V, int32_t F, const int32_t *faces, int64_t *keys, uint32_t *status, d3ga_stream_t stream) {
    D3GA_TRY(tb_check_keys(V, F, faces, keys, status));
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = 3 * (int64_t)F;
    hipLaunchKernelGGL(tb_keys_kernel, dim3((unsigned)tb_blocks(n)), dim3(kBlock), 0, s, V, n, faces, keys, status);
    return check_launch(s, 0);
}

extern "C" int d3ga_loop_plan_scratch_bytes(int32_t V, int32_t F, int64_t *bytes) {
    if (!bytes) return D3GA_E_NULL;
    D3GA_TRY(tb_check_sizes(V, F));
    *bytes = tb_scratch_bytes(V, F);
    return 0;
}

extern "C" int d3ga_loop_plan_build(const d3ga_loop_plan *plan, const int32_t *faces, const int64_t *sorted_keys, const int64_t *perm,
                                    int32_t *info, void *scratch, int64_t scratch_bytes, d3ga_stream_t stream) {
    D3GA_TRY(tb_check_build(plan, faces, sorted_keys, perm, info, scratch, scratch_bytes));
    hipStream_t s = (hipStream_t)stream;
    const int32_t V = plan->V;
    const int64_t n = 3 * (int64_t)plan->F;
    const TbScratch sc = tb_carve(scratch, V, plan->F);
    // valence and cursor lie back to back; the clears are kernels (d3ga_internal.h)
    D3GA_HIP(zero_async(sc.valence, (size_t)(2 * tb_align256(4 * (int64_t)V)), s));
    D3GA_HIP(zero_async(plan->vert_boundary, (size_t)V, s));
    D3GA_HIP(zero_async(info, 8, s));                        // E and the largest valence; the status word is sticky
    hipLaunchKernelGGL(tb_heads_kernel, dim3((unsigned)tb_blocks(n)), dim3(kBlock), 0, s, n, sorted_keys, sc.head);
    D3GA_TRY(tb_scan(n, sc.head, sc.excl, sc, s));
    hipLaunchKernelGGL(tb_edges_kernel, dim3((unsigned)tb_blocks(n)), dim3(kBlock), 0, s, *plan, n, faces, sorted_keys, perm, sc.head, sc.excl,
                       sc.valence, info);
    D3GA_TRY(tb_scan(V, sc.valence, plan->vert_offsets, sc, s));
    hipLaunchKernelGGL(tb_csr_fill_kernel, dim3((unsigned)tb_blocks(n)), dim3(kBlock), 0, s, *plan, info, sc.cursor);
    hipLaunchKernelGGL(tb_csr_sort_kernel, dim3((unsigned)tb_blocks(V)), dim3(kBlock), 0, s, *plan, info);
    return check_launch(s, 0);
}

extern "C" int d3ga_loop_subdivide(const d3ga_loop_plan *plan, int32_t D, const double *x, const double *beta, int32_t n_beta, float *out,
                                   uint32_t *status, d3ga_stream_t stream) {
    D3GA_TRY(tb_check_subdivide(plan, D, x, beta, n_beta, out, status));
    hipStream_t s = (hipStream_t)stream;
    const int64_t total = ((int64_t)plan->V + plan->E) * D;
    if (tb_blocks(total) > INT32_MAX) return D3GA_E_SIZE;
    hipLaunchKernelGGL(tb_stencil_kernel, dim3((unsigned)tb_blocks(total)), dim3(kBlock), 0, s, *plan, D, total, x, beta, n_beta, out, status);
    return check_launch(s, 0);
}

extern "C" int d3ga_loop_faces(const d3ga_loop_plan *plan, const int32_t *faces, int32_t *out, d3ga_stream_t stream) {
    D3GA_TRY(tb_check_faces(plan, faces, out));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(tb_faces_kernel, dim3((unsigned)tb_blocks(plan->F)), dim3(kBlock), 0, s, *plan, faces, out);
    return check_launch(s, 0);
}

extern "C" int d3ga_unpose(int32_t n, int32_t J, int32_t R, int32_t K, const double *vertices, const double *joint_mats, const void *skin_w,
                           int32_t w_f64, const int32_t *skin_idx, const int64_t *rows, const double *offsets, int32_t n_offsets, float *out,
                           uint32_t *status, d3ga_stream_t stream) {
    D3GA_TRY(tb_check_unpose(n, J, R, K, vertices, joint_mats, skin_w, w_f64, skin_idx, rows, offsets, n_offsets, out, status));
    hipStream_t s = (hipStream_t)stream;
    const TbUnpose u = {n, J, R, K, n_offsets, vertices, joint_mats, offsets, skin_idx, rows};
    if (w_f64)
        hipLaunchKernelGGL(tb_unpose_kernel<double>, dim3((unsigned)tb_blocks(n)), dim3(kBlock), 0, s, u, static_cast<const double *>(skin_w), out, status);
    else
        hipLaunchKernelGGL(tb_unpose_kernel<float>, dim3((unsigned)tb_blocks(n)), dim3(kBlock), 0, s, u, static_cast<const float *>(skin_w), out, status);
    return check_launch(s, 0);
}
