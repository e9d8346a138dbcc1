// decimate.hip -- quadric edge-collapse decimation of the cage surface as rounds of independent collapses.  The rules
// are the text of decimate_math.h; this file adds the addressing, the compaction and the launches.  Compiled with -ffp-contract=off:
// the g++ build of that header gives these kernels' bits.
//
//   dc_quadrics     a thread per vertex: the area-weighted plane quadrics of its faces, gathered in ascending face index.
//   dc_clear        a thread per vertex: owner = none, remap = identity; thread 0 clears the count of valid edges.
//   dc_candidates   a thread per edge: link condition, placement, flip test and key.  The neighbour and star loops run per lane (a list
//                   may be longer than a wavefront); the valid edges are counted per workgroup and added with ONE integer atomic each.
//   dc_claim        a thread per admitted edge: 64-bit integer atomicMin of its key into the owner cells of both ends.
//   dc_select       a thread per admitted edge: the test over both closed neighbourhoods; the winner applies its collapse -- its
//                   ends lie in no other winner's closed neighbourhood, so no two winners touch the same vertex.
//   dc_faces_*      a thread per face: relabel, count (wave_prims.h block scan), ONE workgroup over the block totals, emit in order.
// No float atomics, no host synchronisation, no wait on another workgroup.  The status word is sticky (atomicOr of vector lanes).
#include "d3ga_internal.h"
#include "decimate_math.h"
#include "wave_prims.h"

namespace d3ga {

static_assert(kDcBlock == kBlock, "a scan block is a workgroup");
constexpr int kDcTotalsBlock = 256;
constexpr int kDcWaves = kBlock / 64;

__device__ __forceinline__ void dc_raise(uint32_t *status, uint32_t flags) {
    if (flags) atomicOr(status, flags);
}

__global__ __launch_bounds__(kBlock) void dc_quadrics_kernel(const DcMesh m, double *__restrict__ quadrics, uint32_t *status) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= m.V) return;
    uint32_t flags = 0;
    double q[10];
    dc_vertex_quadric(m, (int32_t)v, q, &flags);
    for (int k = 0; k < 10; ++k) quadrics[10 * v + k] = q[k];
    dc_raise(status, flags);
}

__global__ __launch_bounds__(kBlock) void dc_clear_kernel(const int32_t V, unsigned long long *__restrict__ owner, int32_t *__restrict__ remap,
                                                          int64_t *__restrict__ counts) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v == 0) counts[1] = 0;
    if (v >= V) return;
    owner[v] = kDcNoOwner;
    remap[v] = (int32_t)v;
}

__global__ __launch_bounds__(kBlock) void dc_candidates_kernel(const d3ga_loop_plan p, const DcMesh m, int64_t *__restrict__ keys,
                                                               double *__restrict__ placement, int64_t *counts, uint32_t *status) {
    __shared__ uint32_t s_n[kDcWaves];
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t flags = 0, valid = 0;
    if (e < p.E) {
        double point[3];
        const int64_t key = dc_candidate(p, m, (int32_t)e, point, &flags);
        keys[e] = key;
        for (int c = 0; c < 3; ++c) placement[3 * e + c] = point[c];
        valid = key != kDcBadKey;
    }
    uint32_t total;
    block_excl_scan_u32<kDcWaves>(valid, s_n, &total);
    if (threadIdx.x == 0 && total) atomicAdd(reinterpret_cast<unsigned long long *>(counts + 1), (unsigned long long)total);
    dc_raise(status, flags);
}

__global__ __launch_bounds__(kBlock) void dc_claim_kernel(const d3ga_loop_plan p, const int32_t n_admit, const int64_t *__restrict__ sorted_keys,
                                                          unsigned long long *owner, uint32_t *status) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_admit) return;
    uint32_t flags = 0;
    int64_t key;
    int32_t u, w;
    if (dc_admitted(p, sorted_keys, (int32_t)i, &key, &u, &w, &flags)) {
        atomicMin(owner + u, (unsigned long long)key);
        atomicMin(owner + w, (unsigned long long)key);
    }
    dc_raise(status, flags);
}

// owner is read only here and x, quadrics, remap are written only at a winner's own ends: no lane reads what another writes
__global__ __launch_bounds__(kBlock) void dc_select_kernel(const d3ga_loop_plan p, const int32_t n_admit, const int64_t *__restrict__ sorted_keys,
                                                           const uint64_t *__restrict__ owner, const double *__restrict__ placement, double *x,
                                                           double *quadrics, int32_t *remap, uint32_t *status) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_admit) return;
    uint32_t flags = 0;
    int64_t key;
    int32_t u, w;
    if (dc_admitted(p, sorted_keys, (int32_t)i, &key, &u, &w, &flags) && dc_selected(p, owner, u, w, key, &flags))
        dc_apply(x, quadrics, remap, u, w, placement + 3 * (size_t)dc_key_edge(key));
    dc_raise(status, flags);
}

__global__ __launch_bounds__(kBlock) void dc_faces_count_kernel(const int32_t V, const int32_t F, const int32_t *__restrict__ faces,
                                                                const int32_t *__restrict__ remap, uint32_t *__restrict__ block_total, uint32_t *status) {
    __shared__ uint32_t s_n[kDcWaves];
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t flags = 0, keep = 0;
    int32_t row[3];
    if (f < F) keep = dc_relabel(V, faces, remap, (int32_t)f, row, &flags);
    uint32_t total;
    block_excl_scan_u32<kDcWaves>(keep, s_n, &total);
    if (threadIdx.x == 0) block_total[blockIdx.x] = total;
    dc_raise(status, flags);
}

__global__ __launch_bounds__(kDcTotalsBlock) void dc_faces_starts_kernel(const int64_t nblk, const uint32_t *__restrict__ block_total, uint64_t *block_start,
                                                                         int64_t *counts) {
    __shared__ uint64_t s_wave[kDcTotalsBlock / 64];
    scan_block_totals<kDcTotalsBlock>(nblk, block_total, block_start, s_wave);
    if (threadIdx.x == 0) counts[0] = (int64_t)block_start[nblk];            // lane 0 wrote it
}

__global__ __launch_bounds__(kBlock) void dc_faces_emit_kernel(const int32_t V, const int32_t F, const int32_t *__restrict__ faces,
                                                               const int32_t *__restrict__ remap, const uint64_t *__restrict__ block_start,
                                                               int32_t *__restrict__ out) {
    __shared__ uint32_t s_n[kDcWaves];
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t flags = 0, keep = 0;
    int32_t row[3] = {0, 0, 0};
    if (f < F) keep = dc_relabel(V, faces, remap, (int32_t)f, row, &flags);
    uint32_t total;
    const uint32_t before = block_excl_scan_u32<kDcWaves>(keep, s_n, &total);
    if (!keep) return;
    const int64_t at = (int64_t)block_start[blockIdx.x] + before;
    if (at >= F) return;                                     // never: the kept faces are a subset
    for (int c = 0; c < 3; ++c) out[3 * at + c] = row[c];
}

static inline unsigned dc_grid(int64_t n) { return (unsigned)dc_blocks(n < 1 ? 1 : n); }
static inline DcMesh dc_mesh(const d3ga_loop_plan *plan, const d3ga_decimate_desc *d) {
    return {plan->V, plan->F, d->x, d->quadrics, d->faces, d->csr_offsets, d->csr_faces};
}

}  // namespace d3ga

using namespace d3ga;

extern "C" int d3ga_decimate_scratch_bytes(int32_t F, int64_t *bytes) {
    if (!bytes) return D3GA_E_NULL;
    if (F <= 0 || 6 * (int64_t)F > INT32_MAX) return D3GA_E_SIZE;
    *bytes = dc_scratch_bytes(F);
    return 0;
}

extern "C" int d3ga_decimate_quadrics(const d3ga_loop_plan *plan, const d3ga_decimate_desc *desc, d3ga_stream_t stream) {
    D3GA_TRY(dc_check_quadrics(plan, desc));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(dc_quadrics_kernel, dim3(dc_grid(plan->V)), dim3(kBlock), 0, s, dc_mesh(plan, desc), desc->quadrics, desc->status);
    return check_launch(s, 0);
}

extern "C" int d3ga_decimate_candidates(const d3ga_loop_plan *plan, const d3ga_decimate_desc *desc, d3ga_stream_t stream) {
    D3GA_TRY(dc_check_candidates(plan, desc));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(dc_clear_kernel, dim3(dc_grid(plan->V)), dim3(kBlock), 0, s, plan->V, reinterpret_cast<unsigned long long *>(desc->owner), desc->remap,
                       desc->counts);
    hipLaunchKernelGGL(dc_candidates_kernel, dim3(dc_grid(plan->E)), dim3(kBlock), 0, s, *plan, dc_mesh(plan, desc), desc->keys, desc->placement,
                       desc->counts, desc->status);
    return check_launch(s, 0);
}

extern "C" int d3ga_decimate_collapse(const d3ga_loop_plan *plan, const d3ga_decimate_desc *desc, d3ga_stream_t stream) {
    D3GA_TRY(dc_check_collapse(plan, desc));
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = dc_grid(desc->n_admit);
    hipLaunchKernelGGL(dc_claim_kernel, dim3(blocks), dim3(kBlock), 0, s, *plan, desc->n_admit, desc->sorted_keys,
                       reinterpret_cast<unsigned long long *>(desc->owner), desc->status);
    hipLaunchKernelGGL(dc_select_kernel, dim3(blocks), dim3(kBlock), 0, s, *plan, desc->n_admit, desc->sorted_keys, desc->owner, desc->placement, desc->x,
                       desc->quadrics, desc->remap, desc->status);
    return check_launch(s, 0);
}

extern "C" int d3ga_decimate_faces(const d3ga_loop_plan *plan, const d3ga_decimate_desc *desc, d3ga_stream_t stream) {
    D3GA_TRY(dc_check_faces(plan, desc));
    hipStream_t s = (hipStream_t)stream;
    const int64_t nblk = dc_blocks(plan->F);
    const DcScratch sc = dc_carve(desc->scratch, plan->F);
    hipLaunchKernelGGL(dc_faces_count_kernel, dim3((unsigned)nblk), dim3(kBlock), 0, s, plan->V, plan->F, desc->faces, desc->remap, sc.block_total, desc->status);
    hipLaunchKernelGGL(dc_faces_starts_kernel, dim3(1), dim3(kDcTotalsBlock), 0, s, nblk, sc.block_total, sc.block_start, desc->counts);
    hipLaunchKernelGGL(dc_faces_emit_kernel, dim3((unsigned)nblk), dim3(kBlock), 0, s, plan->V, plan->F, desc->faces, desc->remap, sc.block_start, desc->faces_out);
    return check_launch(s, 0);
}
