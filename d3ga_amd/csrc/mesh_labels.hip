// mesh_labels.hip -- part-label transfer onto a body mesh: the reference's lib/segmentation.py::Segmenter.run
// between the rasterizer's fragments and face_to_label.npy, and lib/cage.py::grow_mask_region, as integer kernels with exact,
// reproducible results.  The rules are the text of mesh_labels_math.h; this file adds the addressing only.
//
//   label_mark    launch (a) of the vote, per pixel: an unsigned atomicMax of 1 + y W + x into cell (view, face).  Integer max
//                 does not depend on the order of arrival, which is what the reference's `colors[ids] += rgb` lacks.  A
//                 wavefront owns 64 consecutive pixels of ONE row, and a pixel whose right neighbour (the next lane's pixel,
//                 fetched with a lane shift) shows the same face is dominated by it and sends nothing: a run of equal faces
//                 inside a wavefront costs one atomic (4.4 against 26.8 us at 747 x 1022).  A pixel per lane:
//                 four per lane from 16-byte loads measured slower (14.3 against 12.9 us at 1080p, B = 4) and was not kept.
//   label_tally   launch (b), a thread per face over the views in order: reads the label at the winning pixel, adds into the
//                 face's own histogram row (no atomic) and writes the cell back to 0, so the scratch is clean for the next
//                 call without a clear launch and a captured call can be replayed.
//   label_majority, label_median, label_grow   a thread per face; growth is a two-hop pull from the ring's input mask, so it
//                 needs neither atomics nor a second pass, and all rings of a call are enqueued at once.
#include "d3ga_internal.h"
#include "mesh_labels_math.h"
#include "wave_prims.h"

namespace d3ga {

// a wavefront per row segment, as sample_prep.hip: lane == threadIdx.x, consecutive lanes, consecutive addresses
constexpr int kMarkBlockX = 64, kMarkBlockY = 4;
static_assert(kMarkBlockX * kMarkBlockY == kBlock, "256 threads");

// Every lane of a wavefront reaches the shift (it reads the next lane's register); a lane outside the image holds -1.
__global__ __launch_bounds__(kBlock) void label_mark_kernel(const MlVote v, const int suppress) {
    const int x = blockIdx.x * kMarkBlockX + threadIdx.x, y = blockIdx.y * kMarkBlockY + threadIdx.y, b = blockIdx.z;
    const bool inside = x < v.W && y < v.H;
    const int32_t f = inside ? v.pix_to_face[((size_t)b * v.H + y) * v.W + x] : -1;
    const int32_t next = wave_next_lane(f, -1);
    if (ml_sends(f, next, v.F, suppress != 0)) atomicMax(v.cells + (size_t)b * v.F + f, ml_key(y, x, v.W));
}

__global__ __launch_bounds__(kBlock) void label_tally_kernel(const MlVote v) {
    const int f = blockIdx.x * kBlock + threadIdx.x;
    if (f >= v.F) return;
    if (ml_tally_face(v, f)) atomicOr(v.status, (uint32_t)D3GA_LABEL_STATUS_RANGE);
}

__global__ __launch_bounds__(kBlock) void label_majority_kernel(int F, int L, const int32_t *__restrict__ hist, int32_t *__restrict__ labels) {
    const int f = blockIdx.x * kBlock + threadIdx.x;
    if (f < F) labels[f] = ml_majority(hist + (size_t)f * L, L);
}

__global__ __launch_bounds__(kBlock) void label_median_kernel(int F, const int32_t *__restrict__ neighbours, const int32_t *__restrict__ labels,
                                                              int32_t *__restrict__ out) {
    const int f = blockIdx.x * kBlock + threadIdx.x;
    if (f < F) out[f] = ml_median(neighbours, labels, f, F);
}

__global__ __launch_bounds__(kBlock) void label_grow_kernel(int F, const int32_t *__restrict__ neighbours, const uint8_t *__restrict__ mask,
                                                            uint8_t *__restrict__ out) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j < F) out[j] = ml_grow_face(neighbours, mask, j, F);
}

__global__ __launch_bounds__(kBlock) void label_mask_copy_kernel(int F, const uint8_t *__restrict__ mask, uint8_t *__restrict__ out) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j < F) out[j] = mask[j] != 0;
}

// a lane per face, no stride: every face gets its workgroup (3 F <= INT32_MAX)
static inline dim3 faces_grid(int F) { return dim3(grid_1d(F, INT32_MAX)); }

}  // namespace d3ga

using namespace d3ga;

extern "C" int d3ga_label_vote(int32_t B, int32_t F, int32_t L, int32_t H, int32_t W, const int32_t *pix_to_face, const void *labels,
                               int32_t label_u8, int64_t label_pitch, int64_t label_frame, uint32_t *cells, int32_t *hist, uint32_t *status,
                               int32_t flags, d3ga_stream_t stream) {
    MlVote v;
    D3GA_TRY(ml_plan_vote(B, F, L, H, W, pix_to_face, labels, label_u8, label_pitch, label_frame, cells, hist, status, flags, &v));
    hipStream_t s = (hipStream_t)stream;
    const int suppress = !(flags & D3GA_LABEL_EVERY_PIXEL);
    const dim3 grid((unsigned)((W + kMarkBlockX - 1) / kMarkBlockX), (unsigned)((H + kMarkBlockY - 1) / kMarkBlockY), (unsigned)B);
    const dim3 block(kMarkBlockX, kMarkBlockY);
    hipLaunchKernelGGL(label_mark_kernel, grid, block, 0, s, v, suppress);
    hipLaunchKernelGGL(label_tally_kernel, faces_grid(F), dim3(kBlock), 0, s, v);
    return check_launch(s, 0);
}

extern "C" int d3ga_label_majority(int32_t F, int32_t L, const int32_t *hist, int32_t *labels, d3ga_stream_t stream) {
    D3GA_TRY(ml_check_majority(F, L, hist, labels));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(label_majority_kernel, faces_grid(F), dim3(kBlock), 0, s, F, L, hist, labels);
    return check_launch(s, 0);
}

extern "C" int d3ga_label_median(int32_t F, const int32_t *neighbours, const int32_t *labels, int32_t *out, d3ga_stream_t stream) {
    D3GA_TRY(ml_check_median(F, neighbours, labels, out));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(label_median_kernel, faces_grid(F), dim3(kBlock), 0, s, F, neighbours, labels, out);
    return check_launch(s, 0);
}

extern "C" int d3ga_label_grow(int32_t F, int32_t n_rings, const int32_t *neighbours, const uint8_t *mask, uint8_t *out, uint8_t *scratch,
                               d3ga_stream_t stream) {
    D3GA_TRY(ml_check_grow(F, n_rings, neighbours, mask, out, scratch));
    hipStream_t s = (hipStream_t)stream;
    if (n_rings == 0) hipLaunchKernelGGL(label_mask_copy_kernel, faces_grid(F), dim3(kBlock), 0, s, F, mask, out);
    for (int r = 0; r < n_rings; ++r)
        hipLaunchKernelGGL(label_grow_kernel, faces_grid(F), dim3(kBlock), 0, s, F, neighbours, ml_ring_src(r, mask, scratch, F),
                           ml_ring_dst(r, n_rings, out, scratch, F));
    return check_launch(s, 0);
}
