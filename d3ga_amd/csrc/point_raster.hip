// point_raster.hip -- forward-only point-cloud rasterizer and compositor behind the reference's recorder/pc_renderer.py::PCRenderer
// (pytorch3d PointsRasterizer with points_per_pixel K + AlphaCompositor).  Semantics: DESIGN.md 4.4h; per-element arithmetic:
// point_raster_math.h.  Compiled with -ffp-contract=off and correctly rounded division: the device evaluates the header as
// its g++ build does.
//
// A gather over 16 x 16-pixel tiles (a per-pixel list of the K nearest cannot be kept with atomics).  d3ga_points_rasterize,
// six launches, no host synchronisation, no float atomics:
//   points_clear_kernel    every tile's count := 0 (scratch is never assumed clean).
//   points_count_kernel    one lane per (b, point): project, drop, the tiles its box of pixel centres touches; one integer
//                          atomic add per touched tile and wavefront (the lanes that name one tile elect a leader).
//   points_local_kernel    one lane per tile: the exclusive prefix of the counts inside a workgroup of 256 tiles and its total.
//   points_scan_kernel     one workgroup: exclusive 64-bit prefix of the workgroups' totals.
//   points_scatter_kernel  one lane per (b, point): the projection again (12 bytes read instead of a 24-byte record written and
//                          read), one 16-byte record (u, v, z, index) per touched tile; the slot inside the tile's list is
//                          what an atomic decrement of the tile's count returns, so the order inside a list is arbitrary --
//                          the selection below is a total order over (float_bits(z), index) and does not depend on it.
//   points_tile_kernel<K>  one 256-lane workgroup per (view, tile), one lane per pixel: the list goes through LDS in batches
//                          of 256 records (one 16-byte load per lane, then every lane reads every record: one address per
//                          wavefront, a broadcast); a record whose disc cannot reach the wavefront's four rows is skipped;
//                          each lane keeps its K smallest keys and their dist2 in registers (3 K of them) by an unrolled
//                          insertion and writes its K fragments.
// The lists live in a buffer whose size is a closed-form bound (point_tiles_per_axis(r_px)^2 records per point, at most the
// tiles of the frame), so nothing can overflow; every list access is checked against that capacity all the same.
// d3ga_points_composite is a per-pixel gather over the fragments.
#include "d3ga_internal.h"
#include "point_raster_math.h"
#include "wave_prims.h"

namespace d3ga {

constexpr int kPointBatch = kBlock;             // records per LDS batch of the tile kernel
constexpr int kPointScanBlock = 1024;
constexpr int kPointMaxGrid = 1 << 16;          // workgroups of a grid-stride kernel

struct PointScratch {
    uint32_t *count;         // nblk * kBlock: records per tile (view-major); counted up by count, down to 0 again by scatter
    uint32_t *local;         // nblk * kBlock: exclusive prefix of count inside a workgroup of kBlock tiles
    uint32_t *block_total;   // nblk
    uint64_t *block_start;   // nblk + 1: exclusive prefix of block_total; [nblk] = all records
    PointRec *list;          // capacity
};
static inline int64_t point_tiles(int64_t H, int64_t W) { return ((H + kPointTile - 1) / kPointTile) * ((W + kPointTile - 1) / kPointTile); }
static inline int64_t point_blocks(int64_t B, int64_t H, int64_t W) { return (B * point_tiles(H, W) + kBlock - 1) / kBlock; }
// records the lists can hold at most; < 0: more than this library accepts
static inline int64_t point_capacity(int64_t B, int64_t P, int64_t H, int64_t W, float radius) {
    const int64_t per_axis = point_tiles_per_axis(point_radius_px(radius, (int)H, (int)W));
    const int64_t tiles = point_tiles(H, W);
    const int64_t per_point = per_axis * per_axis < tiles ? per_axis * per_axis : tiles;      // per_axis <= 8194: no overflow
    if (B * P > 0 && per_point > (((int64_t)1 << 36) / (B * P))) return -1;                    // 2^36 records = 1 TiB
    return B * P * per_point;
}
static inline int64_t point_scratch_bytes(int64_t B, int64_t H, int64_t W, int64_t capacity) {
    const int64_t nblk = point_blocks(B, H, W);
    return 2 * align256(4 * nblk * kBlock) + align256(4 * nblk) + align256(8 * (nblk + 1)) + align256((int64_t)sizeof(PointRec) * capacity);
}
static inline PointScratch carve_points(void *base, int64_t B, int64_t H, int64_t W) {
    const int64_t nblk = point_blocks(B, H, W);
    char *p = (char *)base;
    PointScratch s;
    s.count = (uint32_t *)p;        p += align256(4 * nblk * kBlock);
    s.local = (uint32_t *)p;        p += align256(4 * nblk * kBlock);
    s.block_total = (uint32_t *)p;  p += align256(4 * nblk);
    s.block_start = (uint64_t *)p;  p += align256(8 * (nblk + 1));
    s.list = (PointRec *)p;
    return s;
}

struct PointFrame {
    int H, W, tiles_x, tiles_y;
    float r_px, s2, r2;
};

static __global__ __launch_bounds__(kBlock) void points_clear_kernel(uint32_t *__restrict__ count, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) count[i] = 0u;
}

// the record and the tile rectangle of point g of the batch; -> tiles touched
static __device__ __forceinline__ int points_project(int64_t g, int P, const PointFrame &fr, const float *__restrict__ points,
                                                     const float *__restrict__ cams, PointRec *r, int *tx0, int *ty0, int *tx1, int *ty1,
                                                     int64_t *b) {
    *b = g / P;
    float c[kMeshCam], x[3];
#pragma unroll
    for (int k = 0; k < kMeshCam; ++k) c[k] = cams[kMeshCam * *b + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = points[3 * g + k];
    return point_setup(c, x, (uint32_t)(g - *b * P), fr.H, fr.W, fr.r_px, r, tx0, ty0, tx1, ty1);
}

// One atomic per distinct tile among the wavefront's lanes, not one per lane: consecutive points are neighbours in space (the
// Gaussians are stored in tetrahedron order), so the 64 lanes of a wavefront name a handful of tiles, and 64 atomics on one
// address execute one after the other.  Every lane of the wavefront must call this (active: the lane has a tile t).  The groups
// of equal tiles are found with ballots alone; then the leaders of all groups issue their atomics in ONE instruction (a loop
// with a returning atomic per group would wait a memory round trip per group).  kSubtract: the leader takes the group's size
// off count[t] and every lane gets what the counter held before minus its rank inside the group (a distinct value for every
// lane of the group); otherwise the leader adds the size and nothing is returned (no lane waits for the atomic).
template <bool kSubtract>
static __device__ __forceinline__ uint32_t wave_tile_atomic(bool active, int64_t t, uint32_t *count) {
    const int lane = threadIdx.x & 63;
    const uint64_t below = ((uint64_t)1 << lane) - 1;
    int my_leader = lane;
    uint32_t rank = 0, size = 0;
    bool pending = active;
    uint64_t todo = __ballot(pending);
    while (todo) {                               // wave-uniform: one trip per distinct tile
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)t, leader);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)t >> 32), leader);
        const bool mine = pending && (uint64_t)t == (((uint64_t)hi << 32) | lo);
        const uint64_t same = __ballot(mine);
        if (mine) {
            my_leader = leader;
            rank = (uint32_t)__popcll(same & below);
            size = (uint32_t)__popcll(same);
            pending = false;
        }
        todo &= ~same;
    }
    if (!kSubtract) {
        if (active && lane == my_leader) atomicAdd(count + t, size);
        return 0;
    }
    uint32_t before = 0;
    if (active && lane == my_leader) before = atomicSub(count + t, size);
    return __shfl(before, my_leader) - rank;
}

// the t-th tile (row by row) of a tile rectangle that is w tiles wide
static __device__ __forceinline__ int64_t points_rect_tile(int64_t base, int tiles_x, int tx0, int ty0, int w, int k) {
    const int r = k / w;
    return base + (int64_t)(ty0 + r) * tiles_x + tx0 + (k - r * w);
}

static __global__ __launch_bounds__(kBlock) void points_count_kernel(int64_t BP, int P, PointFrame fr, const float *__restrict__ points,
                                                                     const float *__restrict__ cams, uint32_t *count) {
    const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    PointRec r;
    int tx0 = 0, ty0 = 0, tx1 = 0, ty1 = 0, n = 0;
    int64_t b = 0;
    if (g < BP) n = points_project(g, P, fr, points, cams, &r, &tx0, &ty0, &tx1, &ty1, &b);
    const int64_t base = b * fr.tiles_x * fr.tiles_y;
    const int w = tx1 - tx0 + 1;
    for (int k = 0; __ballot(k < n) != 0; ++k)   // no lane leaves before the wavefront is done: the ballots need all 64
        wave_tile_atomic<false>(k < n, points_rect_tile(base, fr.tiles_x, tx0, ty0, w, k), count);
}

static __global__ __launch_bounds__(kBlock) void points_local_kernel(const uint32_t *__restrict__ count, uint32_t *__restrict__ local,
                                                                     uint32_t *__restrict__ block_total) {
    __shared__ uint32_t s_wave[kBlock / 64];
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t total;                              // (count holds nblk * kBlock words, the padding cleared with the rest)
    local[t] = block_excl_scan_u32<kBlock / 64>(count[t], s_wave, &total);
    if (threadIdx.x == 0) block_total[blockIdx.x] = total;
}

static __global__ __launch_bounds__(kPointScanBlock) void points_scan_kernel(int64_t nblk, const uint32_t *__restrict__ block_total,
                                                                             uint64_t *__restrict__ block_start) {
    __shared__ uint64_t s_wave[kPointScanBlock / 64];
    scan_block_totals<kPointScanBlock>(nblk, block_total, block_start, s_wave);
}

static __global__ __launch_bounds__(kBlock) void points_scatter_kernel(int64_t BP, int P, PointFrame fr, int64_t capacity,
                                                                       const float *__restrict__ points, const float *__restrict__ cams,
                                                                       uint32_t *count, const uint32_t *__restrict__ local,
                                                                       const uint64_t *__restrict__ block_start, PointRec *__restrict__ list) {
    const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    PointRec r;
    int tx0 = 0, ty0 = 0, tx1 = 0, ty1 = 0, n = 0;
    int64_t b = 0;
    if (g < BP) n = points_project(g, P, fr, points, cams, &r, &tx0, &ty0, &tx1, &ty1, &b);
    const int64_t base = b * fr.tiles_x * fr.tiles_y;
    const int w = tx1 - tx0 + 1;
    for (int k = 0; __ballot(k < n) != 0; ++k) {
        const int64_t t = points_rect_tile(base, fr.tiles_x, tx0, ty0, w, k);
        const uint32_t before = wave_tile_atomic<true>(k < n, t, count);   // this tile's count was raised once for this point
        if (k < n) {
            const uint64_t pos = block_start[t / kBlock] + local[t] + (uint64_t)(before - 1u);
            if (before != 0u && pos < (uint64_t)capacity) list[pos] = r;
        }
    }
}

template <int K>
static __global__ __launch_bounds__(kBlock) void points_tile_kernel(int64_t n_tiles, int64_t nblk, PointFrame fr, int64_t capacity,
                                                                    const uint32_t *__restrict__ local,
                                                                    const uint64_t *__restrict__ block_start,
                                                                    const PointRec *__restrict__ list, int32_t *__restrict__ idx,
                                                                    float *__restrict__ zbuf, float *__restrict__ dists) {
    __shared__ PointRec s_rec[kPointBatch];
    const int tid = threadIdx.x;
    const int64_t per_view = (int64_t)fr.tiles_x * fr.tiles_y;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {         // the same trip count in every lane: barriers inside
        const int64_t b = t / per_view, rem = t - b * per_view;
        const int ty = (int)(rem / fr.tiles_x), tx = (int)(rem - (int64_t)ty * fr.tiles_x);
        const int i = tx * kPointTile + (tid & (kPointTile - 1)), j = ty * kPointTile + (tid >> 4);
        const int first_row = ty * kPointTile + (tid >> 6) * 4;
        uint64_t begin = block_start[t / kBlock] + local[t];
        uint64_t end = t + 1 < nblk * kBlock ? block_start[(t + 1) / kBlock] + local[t + 1] : block_start[nblk];
        if (end > (uint64_t)capacity) end = (uint64_t)capacity;
        if (begin > end) begin = end;
        uint64_t key[K];
        float d2[K];
#pragma unroll
        for (int k = 0; k < K; ++k) { key[k] = kPointEmptyKey; d2[k] = -1.f; }
        for (uint64_t at = begin; at < end; at += kPointBatch) {
            const int n = end - at < (uint64_t)kPointBatch ? (int)(end - at) : kPointBatch;
            if (tid < n) s_rec[tid] = list[at + tid];
            __syncthreads();
            for (int q = 0; q < n; ++q) {
                const PointRec r = s_rec[q];
                if (point_rows_miss(r, first_row, fr.r_px)) continue;   // the same for the whole wavefront: its four rows
                point_visit<K>(r, i, j, fr.s2, fr.r2, key, d2);
            }
            __syncthreads();
        }
        if (i < fr.W && j < fr.H) {
            const int64_t p = ((b * fr.H + j) * fr.W + i) * K;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const bool filled = key[k] != kPointEmptyKey;
                idx[p + k] = filled ? (int32_t)(uint32_t)key[k] : -1;
                if (zbuf) zbuf[p + k] = filled ? point_key_depth(key[k]) : -1.f;
                if (dists) dists[p + k] = filled ? d2[k] : -1.f;
            }
        }
    }
}

struct PointBg {
    float v[3];
};

static __global__ __launch_bounds__(kBlock) void points_composite_kernel(int64_t n, int64_t hw, int P, int K, float r2,
                                                                         const int32_t *__restrict__ idx, const float *__restrict__ dists,
                                                                         const float *__restrict__ colors, PointBg bg,
                                                                         float *__restrict__ image) {
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += (int64_t)gridDim.x * kBlock) {
        const int64_t b = p / hw;
        float rgb[3];
        point_composite(K, P, idx + p * K, dists + p * K, r2, colors ? colors + 3 * b * P : nullptr, bg.v, rgb);
        image[3 * p] = rgb[0]; image[3 * p + 1] = rgb[1]; image[3 * p + 2] = rgb[2];
    }
}

template <int K>
static void launch_tiles(int64_t n_tiles, int64_t nblk, const PointFrame &fr, int64_t capacity, const PointScratch &sc, int32_t *idx, float *zbuf,
                         float *dists, hipStream_t s) {
    hipLaunchKernelGGL(points_tile_kernel<K>, dim3((unsigned)(n_tiles > kPointMaxGrid ? kPointMaxGrid : n_tiles)), dim3(kBlock), 0, s, n_tiles,
                       nblk, fr, capacity, sc.local, sc.block_start, sc.list, idx, zbuf, dists);
}

}  // namespace d3ga

using namespace d3ga;

// what every entry point checks first: 0 ok
static inline int point_sizes(int32_t B, int32_t P, int32_t H, int32_t W) {
    if (B < 0 || P < 0) return D3GA_E_SIZE;
    if ((int64_t)B * P >= ((int64_t)1 << 31)) return D3GA_E_SIZE;
    if (H < 1 || W < 1 || H > kMeshMaxSide || W > kMeshMaxSide) return D3GA_E_SIZE;
    return D3GA_OK;
}
static inline int point_settings(int32_t K, float radius) {
    if (K < 1 || K > kPointMaxK) return D3GA_E_CONFIG;
    if (!(radius > 0.f) || !(radius <= 3.0e38f)) return D3GA_E_CONFIG;
    return D3GA_OK;
}

extern "C" int d3ga_points_raster_scratch_bytes(int32_t B, int32_t P, int32_t H, int32_t W, float radius, size_t *bytes) {
    D3GA_TRY(point_sizes(B, P, H, W));
    D3GA_TRY(point_settings(1, radius));
    if (!bytes) return D3GA_E_NULL;
    const int64_t capacity = point_capacity(B, P, H, W, radius);
    if (capacity < 0) return D3GA_E_SIZE;
    *bytes = (size_t)point_scratch_bytes(B, H, W, capacity) + 256;
    return D3GA_OK;
}

extern "C" int d3ga_points_rasterize(int32_t B, int32_t P, int32_t H, int32_t W, int32_t K, float radius, const float *points,
                                     const float *cams, void *scratch, int32_t *idx, float *zbuf, float *dists, d3ga_stream_t stream) {
    D3GA_TRY(point_sizes(B, P, H, W));
    D3GA_TRY(point_settings(K, radius));
    const int64_t capacity = point_capacity(B, P, H, W, radius);
    if (capacity < 0) return D3GA_E_SIZE;
    if (!scratch || !idx || !cams || (P > 0 && !points)) return D3GA_E_NULL;
    if (misaligned(points) || misaligned(cams) || misaligned(scratch, 15) || misaligned(idx) || misaligned(zbuf) ||
        misaligned(dists))
        return D3GA_E_CONFIG;
    if (B == 0) return D3GA_OK;
    hipStream_t s = (hipStream_t)stream;
    PointFrame fr;
    fr.H = H; fr.W = W;
    fr.tiles_x = (W + kPointTile - 1) / kPointTile; fr.tiles_y = (H + kPointTile - 1) / kPointTile;
    fr.r_px = point_radius_px(radius, H, W); fr.s2 = point_ndc_scale2(H, W); fr.r2 = radius * radius;
    const int64_t BP = (int64_t)B * P, n_tiles = (int64_t)B * fr.tiles_x * fr.tiles_y, nblk = point_blocks(B, H, W);
    const PointScratch sc = carve_points(scratch, B, H, W);
    hipLaunchKernelGGL(points_clear_kernel, dim3(grid_1d(nblk * kBlock)), dim3(kBlock), 0, s, sc.count, nblk * kBlock);
    if (BP > 0)
        hipLaunchKernelGGL(points_count_kernel, dim3((unsigned)((BP + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, BP, P, fr, points, cams, sc.count);
    hipLaunchKernelGGL(points_local_kernel, dim3((unsigned)nblk), dim3(kBlock), 0, s, sc.count, sc.local, sc.block_total);
    hipLaunchKernelGGL(points_scan_kernel, dim3(1), dim3(kPointScanBlock), 0, s, nblk, sc.block_total, sc.block_start);
    if (BP > 0)
        hipLaunchKernelGGL(points_scatter_kernel, dim3((unsigned)((BP + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, BP, P, fr, capacity, points, cams,
                           sc.count, sc.local, sc.block_start, sc.list);
    switch (K) {
        case 1: launch_tiles<1>(n_tiles, nblk, fr, capacity, sc, idx, zbuf, dists, s); break;
        case 2: launch_tiles<2>(n_tiles, nblk, fr, capacity, sc, idx, zbuf, dists, s); break;
        case 3: launch_tiles<3>(n_tiles, nblk, fr, capacity, sc, idx, zbuf, dists, s); break;
        case 4: launch_tiles<4>(n_tiles, nblk, fr, capacity, sc, idx, zbuf, dists, s); break;
        case 5: launch_tiles<5>(n_tiles, nblk, fr, capacity, sc, idx, zbuf, dists, s); break;
        case 6: launch_tiles<6>(n_tiles, nblk, fr, capacity, sc, idx, zbuf, dists, s); break;
        case 7: launch_tiles<7>(n_tiles, nblk, fr, capacity, sc, idx, zbuf, dists, s); break;
        default: launch_tiles<8>(n_tiles, nblk, fr, capacity, sc, idx, zbuf, dists, s); break;
    }
    return check_launch(s, 0);
}

extern "C" int d3ga_points_composite(int32_t B, int32_t P, int32_t H, int32_t W, int32_t K, float radius, const int32_t *idx,
                                     const float *dists, const float *colors, const float *bg, float *image, d3ga_stream_t stream) {
    D3GA_TRY(point_sizes(B, P, H, W));
    D3GA_TRY(point_settings(K, radius));
    if (!idx || !dists || !bg || !image) return D3GA_E_NULL;
    if (misaligned(idx) || misaligned(dists) || misaligned(colors) || misaligned(image)) return D3GA_E_CONFIG;
    if (B == 0) return D3GA_OK;
    hipStream_t s = (hipStream_t)stream;
    const int64_t hw = (int64_t)H * W, n = hw * B;
    PointBg b;
    b.v[0] = bg[0]; b.v[1] = bg[1]; b.v[2] = bg[2];
    hipLaunchKernelGGL(points_composite_kernel, dim3(grid_1d(n)), dim3(kBlock), 0, s, n, hw, P, K, radius * radius, idx, dists, colors, b, image);
    return check_launch(s, 0);
}
