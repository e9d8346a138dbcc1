// d3ga_internal.h -- scratch-buffer layout and launch helpers shared by the .hip translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "../../include/d3ga.h"
#include "d3ga_math.h"

namespace d3ga {

constexpr int kBlock = 256;

// the library's debug knobs (include/d3ga.h: D3GA_KNOB_*, d3ga_debug_set): value in effect.  No environment is read anywhere.
int debug_knob(int key);

// deform.hip: the argument rules of the deform backward that runs as the tail of the per-Gaussian raster backward
int deform_tail_check(const d3ga_cage_deform_in *in, const d3ga_cage_deform_grads *gr, const d3ga_cage_deform_route *route);

static inline int64_t align256(int64_t x) { return (x + 255) & ~int64_t(255); }

// Per-Gaussian state written by the preprocess kernel (structure of arrays, 256-byte aligned sections).
// View-batched renders (d3ga_raster_*_views): the arrays hold n_views * P records, view v's Gaussian i at v * P + i.
struct GeomBuf {
    float *depth;       // P      view-space z
    float4 *conic_o;    // P      conic (a,b,c) + opacity
    float4 *rgb_invd;   // P      colour + 1/depth
    uint2 *rect;        // P      tile rectangle packed: x = minx | miny<<16, y = maxx | maxy<<16
    uint8_t *clamped;   // P      bit c set: SH colour channel c was clamped at 0
    float *cov3D;       // P*6    3D covariance built from (scale, rotation); unused with a precomputed one (read from the caller's tensor)
    float4 *xyh;        // P      pixel-space centre | half extents of the alpha >= 1/255 ellipse's bounding box (splat_cull):
                        //        the 16-byte record the compositing forward's first stage tests a list entry with
    float *dcol;        // 9 planes of `dcol_stride` floats: d(SH colour)/d(unit view direction), plane 3 * (direction x, y, z) + channel -- left by
                        //        the forward's staged SH evaluation so that preprocess_bwd need not read the coefficients again (96 MB at C3) for dL/dmean
    int64_t dcol_stride;
};
static inline int64_t geom_bytes(int64_t P) {
    return align256(4 * P) + align256(16 * P) + align256(16 * P) + align256(8 * P) + align256(P) +
           align256(24 * P) + align256(16 * P) + align256(36 * P);
}
static inline GeomBuf carve_geom(void *base, int64_t P) {
    char *p = (char *)base;
    GeomBuf g;
    g.depth = (float *)p;     p += align256(4 * P);
    g.conic_o = (float4 *)p;  p += align256(16 * P);
    g.rgb_invd = (float4 *)p; p += align256(16 * P);
    g.rect = (uint2 *)p;      p += align256(8 * P);
    g.clamped = (uint8_t *)p; p += align256(P);
    g.cov3D = (float *)p;     p += align256(24 * P);
    g.xyh = (float4 *)p;      p += align256(16 * P);
    g.dcol = (float *)p;
    g.dcol_stride = P;
    return g;
}
// the records of view v of a batch (every array advanced by v * P records; the dcol planes keep the batch's stride)
__host__ __device__ static inline GeomBuf geom_view(const GeomBuf &g, int64_t P, int64_t v) {
    GeomBuf o = g;
    const int64_t d = v * P;
    o.depth += d; o.conic_o += d; o.rgb_invd += d; o.rect += d; o.clamped += d; o.cov3D += 6 * d; o.xyh += d; o.dcol += d;
    return o;
}

// Binning state.
struct BinBuf {
    uint32_t *counters;     // 8  (D3GA_CNT_*)
    uint32_t *tile_count;   // tiles       duplicates in slots that preprocess reserved (wavefronts whose tile window fits a record)
    uint32_t *tile_count2;  // tiles       duplicates of the other wavefronts: placed behind the reserved slots through tile_cursor
    uint32_t *vis_part;     // kVisParts x kVisStride   partial counts of visible Gaussians, one per cache line: preprocess adds, the scan sums
    uint32_t *tile_start;   // tiles + 1   exclusive prefix of tile_count + tile_count2
    uint32_t *tile_cursor;  // tiles       tile_start + tile_count, written where tile_count2 is not zero
    uint64_t *keys;         // d_capacity  (depth bits << 32 | gaussian index), grouped by tile
    uint32_t *point_list;   // d_capacity  gaussian indices, per tile ascending (depth, index)
    uint32_t *big_tiles;    // tiles       tiles with 4097..8192 entries (counters[4] of them)
    uint32_t *huge_tiles;   // tiles       tiles with more than 8192 entries: no LDS sort (counters[5])
    uint32_t *mid_tiles;    // tiles       tiles with 2049..4096 entries (counters[6])
    uint32_t *tile_order;   // tiles       tile indices by descending list length (work-ordered dispatch of compositing)
};
constexpr int kVisParts = 32, kVisStride = 32;      // 32 partial counters, 128 bytes apart
constexpr int kUnresvWord = 1;                      // word of vis_part (between two partial counters): not zero if some wavefront of
                                                    // the frame is unreserved -- only then does the scan read tile_count2
static inline int64_t bin_bytes(int64_t tiles, int64_t dcap) {
    return 256 + 2 * align256(4 * tiles) + 4 * kVisParts * kVisStride + align256(4 * (tiles + 1)) + align256(4 * tiles) + align256(8 * dcap) +
           align256(4 * dcap) + 4 * align256(4 * tiles);
}
static inline BinBuf carve_bin(void *base, int64_t tiles, int64_t dcap) {
    char *p = (char *)base;
    BinBuf b;
    b.counters = (uint32_t *)p;    p += 256;
    b.tile_count = (uint32_t *)p;  p += align256(4 * tiles);
    b.tile_count2 = (uint32_t *)p; p += align256(4 * tiles);
    b.vis_part = (uint32_t *)p;    p += 4 * kVisParts * kVisStride;
    b.tile_start = (uint32_t *)p;  p += align256(4 * (tiles + 1));
    b.tile_cursor = (uint32_t *)p; p += align256(4 * tiles);
    b.keys = (uint64_t *)p;        p += align256(8 * dcap);
    b.point_list = (uint32_t *)p;  p += align256(4 * dcap);
    b.big_tiles = (uint32_t *)p;   p += align256(4 * tiles);
    b.huge_tiles = (uint32_t *)p;  p += align256(4 * tiles);
    b.mid_tiles = (uint32_t *)p;   p += align256(4 * tiles);
    b.tile_order = (uint32_t *)p;
    return b;
}

struct ImgBuf {
    float *final_T;        // H*W  (view-batched: n_views images back to back)
    uint32_t *n_contrib;   // H*W   1-based tile-list position of the last contributing Gaussian
    // Per-4x4-block culled lists, written by the compositing forward for its backward (raster_composite_scan.hip):
    // a 16x16 tile has 16 blocks (quadrant q = 0..3, row r = 0..3 of that quadrant's wavefront -> block 4q + r); the
    // list of block b of a tile whose depth-sorted list is [begin, end) occupies blk_list[16*begin + b*(end-begin) ...],
    // entries {1-based position in the tile list, Gaussian index}, front to back; blk_count[16*tile + b] = the length of the
    // prefix that holds every entry some pixel of the block blended -- what the backward walks.
    uint32_t *blk_count;   // 16 * tiles
    uint2 *blk_list;       // 16 * d_capacity
};
// W x H: one view; tiles: of the whole batch; views: images in the batch
static inline int64_t img_bytes(int64_t W, int64_t H, int64_t tiles, int64_t dcap, int64_t views = 1) {
    return 2 * align256(4 * W * H * views) + align256(64 * tiles) + align256(128 * dcap);
}
static inline ImgBuf carve_img(void *base, int64_t W, int64_t H, int64_t tiles, int64_t views = 1) {
    ImgBuf i;
    char *p = (char *)base;
    i.final_T = (float *)p;        p += align256(4 * W * H * views);
    i.n_contrib = (uint32_t *)p;   p += align256(4 * W * H * views);
    i.blk_count = (uint32_t *)p;   p += align256(64 * tiles);
    i.blk_list = (uint2 *)p;
    return i;
}

// ---------------------------------------------------------------------------------------------------------
// Wavefront-private tile window and slot reservation.  The Gaussians are stored in tet order, so the union of the tile
// rectangles of 64 consecutive ones is small (C3, over the bench's eight cameras: p50 9-12, p99 28-80, max 391 tiles).  A wavefront of preprocess counts its duplicates
// with LDS atomics inside that window, in LDS nobody else touches (program order + wave_barrier, no workgroup barrier), and sends
// ONE returning global atomic per touched tile to tile_count: the value it returns is the first slot, within the tile's list, of
// the wavefront's duplicates there.  Box and bases are left in the wavefront's RESERVATION RECORD, and the scatter pass places
// every key with one LDS atomic on  tile_start + base  -- it neither counts nor touches a global counter.
//   record of (view v, wavefront w of the view's launch) = kResvStride words at  (v * resv_waves(P) + w) * kResvStride:
//     [0] x0 | y0 << 16   [1] w | h << 16   (the window in tiles of the batch's grid; w * h == 0: nothing visible)   [2..3] unused
//     [4 + k]  base of window tile k = (ty - y0) * w + (tx - x0), written for every k < w * h (0 where the wavefront has no
//              duplicate): the scatter seeds all cursors of the window from it, so nothing of an earlier frame is ever read
// A window of more than kResvTiles tiles (screen-filling splats) marks the wavefront as UNRESERVED: its duplicates are counted in
// tile_count2 and placed one global atomic each through tile_cursor, behind the reserved slots of the tile.
// ---------------------------------------------------------------------------------------------------------
constexpr int kResvStride = 512;                     // words per record (2 KiB)
constexpr int kResvHdr = 4;
constexpr int kResvTiles = kResvStride - kResvHdr;   // window tiles a record holds: every wavefront of C3 fits (max 391 over the bench's eight cameras)
constexpr int kResvSlots = (kResvTiles + 63) / 64;   // window tiles per lane
static inline int64_t resv_waves(int64_t P) { return (kBlock / 64) * ((P + kBlock - 1) / kBlock); }   // records per view
static inline int64_t resv_bytes(int64_t P, int64_t views) { return align256(4 * kResvStride * resv_waves(P) * views); }

struct TileWindow {
    int x0, y0, w, h;             // window origin and size in tiles; w*h == 0 -> nothing visible in the wavefront
    __device__ __forceinline__ bool empty() const { return w <= 0 || h <= 0; }
    __device__ __forceinline__ bool fits() const { return w <= kResvTiles && h <= kResvTiles && w * h <= kResvTiles; }
    __device__ __forceinline__ int area() const { return w * h; }      // (of a window that fits)
    // window slot k -> global tile index (exact for k < 4096: the fractional part of (k + 0.5) / w is >= 0.5 / w away from
    // an integer, the float error is < 5e-4 / w; a 32-bit integer division costs ~40 instructions)
    __device__ __forceinline__ int tile_of(int k, int gx, float inv_w) const {
        const int r = (int)(((float)k + 0.5f) * inv_w);
        return (y0 + r) * gx + x0 + (k - r * w);
    }
};

#ifdef __HIPCC__
// the union of the wavefront's visible rectangles, by butterfly shuffles: the same in every lane
__device__ __forceinline__ TileWindow wave_tile_window(bool visible, int rx0, int ry0, int rx1, int ry1) {
    int bx0 = visible ? rx0 : 0x7fffffff, by0 = visible ? ry0 : 0x7fffffff, bx1 = visible ? rx1 : 0, by1 = visible ? ry1 : 0;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        bx0 = min(bx0, __shfl_xor(bx0, off)); by0 = min(by0, __shfl_xor(by0, off));
        bx1 = max(bx1, __shfl_xor(bx1, off)); by1 = max(by1, __shfl_xor(by1, off));
    }
    TileWindow win;
    win.x0 = bx0; win.y0 = by0;
    win.w = bx1 > bx0 ? bx1 - bx0 : 0;
    win.h = by1 > by0 ? by1 - by0 : 0;
    if (win.w == 0 || win.h == 0) { win.x0 = 0; win.y0 = 0; win.w = 0; win.h = 0; }
    return win;
}
#endif

static inline int tiles_x(int W) { return (W + kTile - 1) / kTile; }
static inline int tiles_y(int H) { return (H + kTile - 1) / kTile; }
// cameras in the batch (d3ga_raster_params::n_views: 0 and 1 both mean one)
static inline int n_views_of(const d3ga_raster_params *prm) { return prm->n_views > 1 ? prm->n_views : 1; }
// windowed camera slot (d3ga.h: D3GA_CAMERA_SLOT_WINDOWED): W, H are the window, the tile grid has one spare column and row per view
static inline bool is_windowed(const d3ga_raster_params *prm) { return prm->tanfovx == D3GA_CAMERA_SLOT_WINDOWED; }
static inline int grid_x(const d3ga_raster_params *prm) { return tiles_x(prm->W) + (is_windowed(prm) ? 1 : 0); }
static inline int grid_y(const d3ga_raster_params *prm) { return tiles_y(prm->H) + (is_windowed(prm) ? 1 : 0); }
// the window table behind the binning buffer's sections (one int4 {ox, oy, w, h} per view): null unless windowed
static inline int4 *win_table(void *binning, int64_t tiles, int64_t dcap) { return (int4 *)((char *)binning + bin_bytes(tiles, dcap)); }
static inline int64_t win_table_bytes(int64_t views) { return align256(16 * views); }
// the reservation records (resv_bytes) are the last section: behind the window table where there is one
static inline uint32_t *resv_records(void *binning, int64_t tiles, int64_t dcap, int64_t views, bool windowed) {
    return (uint32_t *)((char *)binning + bin_bytes(tiles, dcap) + (windowed ? win_table_bytes(views) : 0));
}

// launch check: returns hipError (>0) or 0; in debug mode also synchronises
static inline int check_launch(hipStream_t s, int debug) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    if (debug) {
        e = hipStreamSynchronize(s);
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

#define D3GA_TRY(expr)            \
    do {                          \
        int _st = (expr);         \
        if (_st != 0) return _st; \
    } while (0)
#define D3GA_HIP(expr)                          \
    do {                                        \
        hipError_t _e = (expr);                 \
        if (_e != hipSuccess) return (int)_e;   \
    } while (0)

// argument checks of the entry points: an address that is no multiple of mask + 1 (null passes: optional arguments)
static inline bool misaligned(const void *p, uintptr_t mask = 3) { return ((uintptr_t)p & mask) != 0; }
static inline bool aligned16(const void *p) { return !misaligned(p, 15); }
// workgroups of a grid-stride kernel with one lane per item: ceil(n / kBlock), at least 1, at most cap
static inline unsigned grid_1d(int64_t n, int64_t cap = 65536) {
    const int64_t blocks = (n + kBlock - 1) / kBlock;
    return (unsigned)(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
}

// What must happen once per device before a kernel's first launch there (function attributes are per device):
//   static PerDeviceOnce once;  D3GA_TRY(once.run([&] { return (int)hipFuncSetAttribute(...); }));
// Entry points are re-entrant across devices and streams (include/d3ga.h), hence atomics: two threads may both run fn, which is
// harmless, and none skips it before it has succeeded.  A device index past the table runs fn on every call.
struct PerDeviceOnce {
    std::atomic<bool> done[64] = {};
    template <typename Fn>
    int run(Fn fn) {
        int dev = 0;
        D3GA_HIP(hipGetDevice(&dev));
        const bool listed = dev >= 0 && dev < 64;
        if (listed && done[dev].load(std::memory_order_acquire)) return 0;
        D3GA_TRY(fn());
        if (listed) done[dev].store(true, std::memory_order_release);
        return 0;
    }
};

// Zero-fill as a KERNEL node.  hipMemsetAsync becomes a memset node under stream capture, and on this stack (ROCm 7.2,
// gfx950) a replayed graph did not reliably order such a node against the kernels around it: with the tile histogram
// zeroed by a memset node, replays of preprocess -> bin_sort faulted as soon as anything disturbed the caches between two
// replays (tools/diag_graph3.py), i.e. the histogram was being zeroed while the next kernel already counted into it.
// Kernel -> kernel edges are honoured, so every clear in this library is a (tiny) kernel.
#ifdef __HIPCC__
static __global__ void zero_words_kernel(uint32_t *__restrict__ p, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = 0u;
}
static __global__ void zero_bytes_kernel(unsigned char *__restrict__ p, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = 0;
}
static inline hipError_t zero_async(void *ptr, size_t bytes, hipStream_t s) {
    if (bytes == 0) return hipSuccess;
    if ((((uintptr_t)ptr | bytes) & 3) == 0) {
        const size_t n = bytes / 4;
        const size_t blocks = (n + 4 * kBlock - 1) / (4 * kBlock);
        hipLaunchKernelGGL(zero_words_kernel, dim3((unsigned)(blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks))), dim3(kBlock), 0, s,
                           reinterpret_cast<uint32_t *>(ptr), n);
    } else {
        const size_t blocks = (bytes + kBlock - 1) / kBlock;
        hipLaunchKernelGGL(zero_bytes_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(kBlock), 0, s,
                           reinterpret_cast<unsigned char *>(ptr), bytes);
    }
    return hipGetLastError();
}
#endif

}  // namespace d3ga
