// raster_pre.hip -- per-Gaussian stages of the tile rasterizer for gfx950.
//
//   preprocess_kernel      project, EWA 2D covariance, conic, radius, tile rectangle, SH colour, tile histogram + slot reservation
//   preprocess_bwd_kernel  conic/mean2D/colour/opacity gradients -> mean3D, cov3D | (scale, rotation), SH
//
// Both are HBM-streaming: one thread per Gaussian, every per-Gaussian array read/written once (algorithmic bytes per
// Gaussian: fwd 88 + 12 M).  The wide (P,M,3) SH arrays go through per-wavefront LDS slabs so that
// global accesses are 16 B per lane and lane-contiguous; the camera matrices are wave-uniform and come through the
// scalar cache.  No MFMA.
#include <type_traits>

#include "composite_common.h"
#include "raster_pre_body.h"
#include "deform_tail.h"

namespace d3ga {

// ---------------------------------------------------------------------------------------------------------
// SH staging.  shs / dL_dsh are (P, M, 3): 12*M bytes per Gaussian, so a thread-per-Gaussian access walks memory with
// a 192-byte stride (M = 16) and every load instruction of a wavefront touches 64 different cache lines -- measured
// 3.5x over-fetch.  Instead each wavefront moves the 64 rows it owns as ONE contiguous block with 16-byte-per-lane,
// lane-contiguous accesses (1 KiB per instruction) through an LDS slab, and every lane then works on its own row in
// LDS.  Rows are padded to 52 floats = 13 x 16 B (odd number of 16-byte slots -> conflict-free b128 row access).
// Used when 3*M is a multiple of 4 floats (M = 4, 8, 12, 16; D3GA always has M = 16); otherwise rows are accessed
// in global memory directly.
// ---------------------------------------------------------------------------------------------------------
constexpr int kShRow = 52;
constexpr int kShSlab = 64 * kShRow;            // floats per wavefront
constexpr size_t kShLdsBytes = (size_t)(kBlock / 64) * kShSlab * sizeof(float);   // 53,248 B per block

__host__ __device__ __forceinline__ bool sh_staged(int M) { return M > 0 && (3 * M) % 4 == 0 && 3 * M <= 48; }

// global (rows x 3M floats, contiguous) -> LDS slab; `rows` valid rows of this wavefront (<= 64)
__device__ __forceinline__ void sh_slab_load(float *slab, const float *__restrict__ src, int rows, int M3, int lane) {
    const int nvec = rows * M3 / 4;
    for (int v = lane; v < nvec; v += 64) {
        const float4 x = reinterpret_cast<const float4 *>(src)[v];
        const int e = 4 * v, r = e / M3, c = e - r * M3;
        *reinterpret_cast<float4 *>(slab + r * kShRow + c) = x;
    }
}
__device__ __forceinline__ void sh_slab_store(const float *slab, float *__restrict__ dst, int rows, int M3, int lane) {
    const int nvec = rows * M3 / 4;
    for (int v = lane; v < nvec; v += 64) {
        const int e = 4 * v, r = e / M3, c = e - r * M3;
        reinterpret_cast<float4 *>(dst)[v] = *reinterpret_cast<const float4 *>(slab + r * kShRow + c);
    }
}

// The common case -- full rows of 48 floats (M = 16) and a full set of ROWS rows -- with every load of the set in flight at
// once: the loop above is one load -> wait -> LDS store per iteration (an integer division by the run-time row length
// sits between them), i.e. ROWS*12/64 memory round trips in series per wavefront, and that chain, not bandwidth, set the
// pace of both per-Gaussian kernels (preprocess 53 -> .. us, preprocess_bwd 58 -> .. us at C3).
template <int ROWS>
struct ShRegs { float4 v[ROWS * 12 / 64]; };
template <int ROWS>
__device__ __forceinline__ ShRegs<ROWS> sh_rows48_load(const float *__restrict__ src, int lane) {
    ShRegs<ROWS> r;
#pragma unroll
    for (int k = 0; k < ROWS * 12 / 64; ++k) r.v[k] = reinterpret_cast<const float4 *>(src)[lane + 64 * k];
    return r;
}
template <int ROWS>
__device__ __forceinline__ void sh_rows48_to_slab(float *slab, const ShRegs<ROWS> &r, int lane) {
#pragma unroll
    for (int k = 0; k < ROWS * 12 / 64; ++k) {
        const int e = 4 * (lane + 64 * k), row = e / 48, c = e - row * 48;
        *reinterpret_cast<float4 *>(slab + row * kShRow + c) = r.v[k];
    }
}
template <int ROWS>
__device__ __forceinline__ void sh_rows48_store(const float *slab, float *__restrict__ dst, int lane) {
#pragma unroll
    for (int k = 0; k < ROWS * 12 / 64; ++k) {
        const int e = 4 * (lane + 64 * k), row = e / 48, c = e - row * 48;
        reinterpret_cast<float4 *>(dst)[lane + 64 * k] = *reinterpret_cast<const float4 *>(slab + row * kShRow + c);
    }
}

// forward staging (see preprocess_kernel): 32 of a wavefront's 64 rows at a time, in two passes
constexpr int kShPassRows = 32;
constexpr int kShHalfSlab = kShPassRows * kShRow;
constexpr size_t kShHalfLdsBytes = (size_t)(kBlock / 64) * kShHalfSlab * sizeof(float);      // 26,624 B per block

// The two passes of a full wavefront of full rows (M = 16) of the training forward, with `before` between the issue of half 0 and
// its use: what the caller has to do that does not need the rows and may use the slab region, which is free until then
// (preprocess_full_wavefront: projection and slot reservation; staged_sh_colour: the basis).
// What the compiler makes of it (ISA of preprocess_kernel<true,false>): the six loads of half 0 are issued right behind the
// caller's mean and opacity loads and are first waited for in front of their slab writes; half 1, issued in the source behind the
// first pass, is six loads and their wait in front of the second pass (ahead of the first pass it costs 24 registers at the kernel's
// peak, 93 -> 107 VGPRs, four wavefronts per SIMD).
// SIX NAMED VALUES per half, not ShRegs: the loads of an array (sh_rows48_load) are sunk to their first use, behind `before` -- the
// forward-only branch of staged_sh_colour relies on exactly that to stay at its 72 VGPRs (with the named values it has 86 and loses
// two wavefronts per SIMD) -- while named values stay where the source has them.  Nothing else holds a load of a `const
// __restrict__` argument in place that does not also change what the vectoriser packs, and with it the rounding (docs/LOG.md).
#define D3GA_SH_HALF_ISSUE(H, SRC)                                                                                        \
    const float4 *H##g = reinterpret_cast<const float4 *>(SRC) + lane;                                                     \
    const float4 H##0 = H##g[0], H##1 = H##g[64], H##2 = H##g[128], H##3 = H##g[192], H##4 = H##g[256], H##5 = H##g[320];
#define D3GA_SH_HALF_TO_SLAB(H)                                                                                           \
    sh_row48_put(slab, lane, H##0); sh_row48_put(slab, lane + 64, H##1); sh_row48_put(slab, lane + 128, H##2);             \
    sh_row48_put(slab, lane + 192, H##3); sh_row48_put(slab, lane + 256, H##4); sh_row48_put(slab, lane + 320, H##5);
static_assert(kShPassRows * 12 / 64 == 6, "six 16-byte loads per lane and half");
// 16-byte piece v of a block of full rows -> its place in the slab (as sh_rows48_to_slab)
__device__ __forceinline__ void sh_row48_put(float *slab, int v, float4 x) {
    const int e = 4 * v, row = e / 48, c = e - row * 48;
    *reinterpret_cast<float4 *>(slab + row * kShRow + c) = x;
}
template <class Before, class Eval>
__device__ __forceinline__ void sh_two_pass48(float *slab, const float *__restrict__ src, int lane, Before &&before, Eval &&eval) {
    D3GA_SH_HALF_ISSUE(h0_, src)
    before();
    __builtin_amdgcn_wave_barrier();
    D3GA_SH_HALF_TO_SLAB(h0_)
    __builtin_amdgcn_wave_barrier();
    if (lane / kShPassRows == 0) eval(slab + (lane % kShPassRows) * kShRow);
    D3GA_SH_HALF_ISSUE(h1_, src + 48 * kShPassRows)
    __builtin_amdgcn_wave_barrier();
    D3GA_SH_HALF_TO_SLAB(h1_)
    __builtin_amdgcn_wave_barrier();
    if (lane / kShPassRows == 1) eval(slab + (lane % kShPassRows) * kShRow);
}
#undef D3GA_SH_HALF_ISSUE
#undef D3GA_SH_HALF_TO_SLAB

// sum_k Y_k(dir_i) * coeff_k of this thread's Gaussian (mean: its means3D row, loaded by the caller; any value for i >= P), with
// the (P,M,3) block read through wavefront-private LDS: into acc, or (WANT_J) into cj.a0..a2 with J = d(colour)/d(unit direction)
// (sh_accumulate_jacobian), from the same staged row.
// SH colour in two PASSES over half of the wavefront's rows each (full 192-byte rows, so every byte is fetched once): the slab
// of a wavefront is 32 x 52 floats, 6.5 KiB (20 resident wavefronts per CU; 64 rows would be 13 KiB and 12).  Round 4
// measured 16 rows per pass (3.3 KiB: the tile window's 16 KiB is then the block's LDS, 28 wavefronts per CU, the launch's
// 1954 workgroups in 1.09 instead of 1.53 rounds): with all four quarters in flight the registers hold the kernel at 20
// wavefronts anyway (88 VGPRs); with two in flight (68 VGPRs, 28 wavefronts) preprocess takes 61-65 us against 55.6 (eager
// stage events, same box) -- the second memory round trip per wavefront and a quarter of the lanes per accumulate pass cost
// more than the occupancy returns (docs/LOG.md).  Only wavefront-private LDS is touched: no workgroup barrier, program order +
// wave_barrier suffice.  Every thread of the block must call it.
template <bool WANT_J>
__device__ __forceinline__ void staged_sh_colour(const d3ga_raster_params &prm, V3 mean, const float *__restrict__ shs,
                                                 const float *__restrict__ campos, float *s_sh, float acc[3], ShColJ &cj) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x * kBlock + tid;
    const int M3 = 3 * prm.M;
    float *slab = s_sh + wave * kShHalfSlab;
    const int row0 = blockIdx.x * kBlock + wave * 64;           // first Gaussian of this wavefront
    const int rows = min(64, prm.P - row0);
    const int nb = (prm.sh_degree + 1) * (prm.sh_degree + 1);
    float B[16];
    float dx = 0.f, dy = 0.f, dz = 1.f;
    auto eval = [&](const float *row) __attribute__((always_inline)) {
        if (WANT_J) cj = sh_accumulate_jacobian(B, dx, dy, dz, row, nb, cj);
        else sh_accumulate(B, row, 0, 16, nb, acc);
    };
    if (M3 == 48 && rows == 64) {                              // wave-uniform: a full wavefront of full rows
        if (WANT_J) {
            sh_two_pass48(slab, shs + (size_t)48 * row0, lane, [&]() __attribute__((always_inline)) {
                sh_view_dir(mean, campos, dx, dy, dz);
                sh_basis(prm.sh_degree, dx, dy, dz, B);
            }, eval);
            return;
        }
        // Forward only, as it was: the source issues both halves up front as arrays, and the compiler sinks each to its use (six
        // loads, their wait, the slab writes, the pass; then the same again) -- which keeps these light kernels at their occupancy:
        // through sh_two_pass48 preprocess_kernel<false,.> has 86 VGPRs instead of 72 (7 -> 5 wavefronts per SIMD).
        const float *src = shs + (size_t)48 * row0;
        const ShRegs<kShPassRows> h0 = sh_rows48_load<kShPassRows>(src, lane);
        const ShRegs<kShPassRows> h1 = sh_rows48_load<kShPassRows>(src + 48 * kShPassRows, lane);
        sh_view_basis(prm, mean, campos, B);
        __builtin_amdgcn_wave_barrier();
        sh_rows48_to_slab<kShPassRows>(slab, h0, lane);
        __builtin_amdgcn_wave_barrier();
        if (lane / kShPassRows == 0) eval(slab + (lane % kShPassRows) * kShRow);
        __builtin_amdgcn_wave_barrier();
        sh_rows48_to_slab<kShPassRows>(slab, h1, lane);
        __builtin_amdgcn_wave_barrier();
        if (lane / kShPassRows == 1) eval(slab + (lane % kShPassRows) * kShRow);
        return;
    }
    if (WANT_J && i < prm.P) sh_view_dir(mean, campos, dx, dy, dz);
    if (i < prm.P) sh_view_basis(prm, mean, campos, B);
    for (int h = 0; h < 2; ++h) {
        const int r = min(kShPassRows, rows - kShPassRows * h);
        __builtin_amdgcn_wave_barrier();
        if (r > 0) sh_slab_load(slab, shs + (size_t)M3 * (row0 + kShPassRows * h), r, M3, lane);
        __builtin_amdgcn_wave_barrier();
        if (i < prm.P && lane / kShPassRows == h) eval(slab + (lane % kShPassRows) * kShRow);
    }
}

// a Gaussian's tile rectangle in the batch's grid (tile_row0: its view's first tile row there)
struct TileRect { bool visible; int r0, r1, r2, r3; };
__device__ __forceinline__ TileRect view_tile_rect(const PreOut &o, int tile_row0) {
    const Splat &sp = o.sp;
    return TileRect{sp.visible, sp.rect[0], sp.rect[1] + tile_row0, sp.rect[2], sp.rect[3] + tile_row0};
}
// d3ga_raster_params::tile_cull (the TC instantiations): the rectangle that goes to the reservation and into geom.rect is the
// reference's cut down to the tiles the splat's alpha >= 1/255 box reaches (d3ga_math.h: tile_rect_tight), from the half extents
// the compositing forward's stage one tests with -- the splat_cull() whose result write_geom_records_splat stores.  On the view's
// own raster, so in front of a window clip.  Nothing else of the splat moves.
__device__ __forceinline__ void tile_tighten(PreOut &o) {
    Splat &sp = o.sp;
    if (!sp.visible) return;
    const SplatCull sc = splat_cull(sp.conic[0], sp.conic[1], sp.conic[2], o.opacity);
    tile_rect_tight(sp.rect, sp.px, sp.py, sc.hx, sc.hy, sp.rect);
}
// what preprocess leaves per Gaussian (GeomBuf records of ITS view, radius), in two parts: what the projection alone decides, and
// what needs the colour.  preprocess_kernel's full wavefronts store the first part before the SH passes, so that the splat does not
// sit in registers through them; 1 / depth and the visibility are what the second part keeps of it.
__device__ __forceinline__ float write_geom_records_splat(const GeomBuf &geom, int i, const PreOut &o, bool keep_cov, int tile_row0,
                                                          int32_t *__restrict__ radii) {
    const Splat &sp = o.sp;
    if (keep_cov) {                         // (uniform) a precomputed covariance is read again from the caller's tensor
#pragma unroll
        for (int k = 0; k < 6; ++k) geom.cov3D[6 * (size_t)i + k] = o.c6[k];
    }
    radii[i] = sp.radius;
    geom.depth[i] = sp.depth;
    // culled Gaussians keep an EMPTY rectangle: the scatter pass and the backward test visibility through it
    geom.rect[i] = sp.visible ? make_uint2((uint32_t)sp.rect[0] | ((uint32_t)(sp.rect[1] + tile_row0) << 16),
                                           (uint32_t)sp.rect[2] | ((uint32_t)(sp.rect[3] + tile_row0) << 16))
                              : make_uint2(0u, 0u);
    geom.conic_o[i] = make_float4(sp.conic[0], sp.conic[1], sp.conic[2], o.opacity);
    {   // half extents of the splat's alpha >= 1/255 box, by the function the compositing stage culls with (bit-identical)
        const SplatCull sc = splat_cull(sp.conic[0], sp.conic[1], sp.conic[2], o.opacity);
        geom.xyh[i] = make_float4(sp.px, sp.py, sp.visible ? sc.hx : -1.0f, sc.hy);
    }
    return sp.visible ? 1.0f / sp.depth : 0.f;
}
__device__ __forceinline__ void write_geom_records_colour(const GeomBuf &geom, int i, float r, float g, float b, float invd,
                                                           uint8_t clampmask, bool want_j, const ShColJ &cj) {
    geom.rgb_invd[i] = make_float4(r, g, b, invd);
    geom.clamped[i] = clampmask;
    if (want_j) dcol_store(geom.dcol, geom.dcol_stride, i, cj);
}
__device__ __forceinline__ void write_geom_records(const GeomBuf &geom, int i, const PreOut &o, bool keep_cov, int tile_row0,
                                                   int32_t *__restrict__ radii, bool want_j, const ShColJ &cj) {
    const float invd = write_geom_records_splat(geom, i, o, keep_cov, tile_row0, radii);
    write_geom_records_colour(geom, i, o.rgb[0], o.rgb[1], o.rgb[2], invd, o.clampmask, want_j, cj);
}

// Windowed camera slot (d3ga.h: D3GA_CAMERA_SLOT_WINDOWED): the splat was projected on the view's full raster; its tile rectangle
// is intersected with the window's tiles [x0, x0 + gx) x [y0, y0 + gy) and rebased to them.  Only integer tile indices move: every
// float of the record is the full-raster one.  A rectangle that misses the window culls the Gaussian in this view (radius kept).
__device__ __forceinline__ PreOut window_clip(PreOut o, int x0, int y0, int gx, int gy) {
    Splat &sp = o.sp;
    const int r0 = max(sp.rect[0], x0) - x0, r1 = max(sp.rect[1], y0) - y0;
    const int r2 = min(sp.rect[2], x0 + gx) - x0, r3 = min(sp.rect[3], y0 + gy) - y0;
    if (sp.visible && r2 > r0 && r3 > r1) { sp.rect[0] = r0; sp.rect[1] = r1; sp.rect[2] = r2; sp.rect[3] = r3; }
    else { sp.visible = false; sp.rect[0] = sp.rect[1] = sp.rect[2] = sp.rect[3] = 0; }
    return o;
}
// the window table of the binning buffer (one {ox, oy, w, h} per view) from the views' 9-float camera rows
__global__ void window_table_kernel(d3ga_raster_params prm, const float *__restrict__ campos, int views, int4 *__restrict__ table) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= views) return;
    const ViewCam c = view_cam(prm, nullptr, nullptr, campos + (size_t)D3GA_CAMERA_SLOT_WINDOWED_FLOATS * v, true);
    table[v] = make_int4(c.ox, c.oy, c.W, c.H);
}

// Tile histogram (counting-sort pass 1) and slot reservation of ONE WAVEFRONT's Gaussians (d3ga_internal.h: reservation records),
// in two steps so that the round trip of the returning atomics runs under what the caller puts between them (preprocess_kernel's
// full wavefronts: the SH passes and the record stores; otherwise the record stores alone).
// s_win: kResvTiles words of LDS that only this wavefront touches (program order + wave_barrier order its accesses); every lane of
// the wavefront must call both.
struct TileResv { TileWindow win; uint32_t base[kResvSlots]; };
template <bool SCALAR_WIN = false /* the caller carries the window through long code: keep it in scalar registers */>
__device__ __forceinline__ TileResv tile_reserve_issue(uint32_t *s_win, const TileRect &t, int gx, uint32_t *__restrict__ tile_count,
                                                       uint32_t *__restrict__ tile_count2, uint32_t *__restrict__ vis_part) {
    const int lane = threadIdx.x & 63;
    TileResv r;
    r.win = wave_tile_window(t.visible, t.r0, t.r1, t.r2, t.r3);
    // the same in every lane: told to the compiler, the window lives in scalar registers from here to tile_reserve_store (four
    // vector registers less through the SH passes of preprocess_full_wavefront, which is what keeps it at five wavefronts per SIMD)
    if constexpr (SCALAR_WIN) {
    r.win.x0 = __builtin_amdgcn_readfirstlane(r.win.x0); r.win.y0 = __builtin_amdgcn_readfirstlane(r.win.y0);
    r.win.w = __builtin_amdgcn_readfirstlane(r.win.w); r.win.h = __builtin_amdgcn_readfirstlane(r.win.h);
    }
#pragma unroll
    for (int j = 0; j < kResvSlots; ++j) r.base[j] = 0u;
    // the visible count: one popcount and one atomic per wavefront, spread over kVisParts cache lines that the scan workgroup sums.
    // (Into counters[D3GA_CNT_VISIBLE] directly -- 7813 adds to ONE address at C3 -- the counter was the kernel's critical path:
    // same-address atomics are served one after the other, preprocess 57 -> 122 us; LOG "Binning: slots reserved in preprocess".)
    const unsigned long long vis = __ballot(t.visible);
    if (lane == 0 && vis) atomicAdd(&vis_part[((blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) % kVisParts) * kVisStride], (uint32_t)__popcll(vis));
    if (r.win.empty()) return r;                             // uniform
    if (r.win.fits()) {
        const int area = r.win.area();
        __builtin_amdgcn_wave_barrier();                     // (whatever the wavefront read from this LDS before)
#pragma unroll
        for (int j = 0; j < kResvSlots; ++j)
            if (lane + 64 * j < area) s_win[lane + 64 * j] = 0u;
        __builtin_amdgcn_wave_barrier();
        if (t.visible)
            for (int ty = t.r1; ty < t.r3; ++ty)
                for (int tx = t.r0; tx < t.r2; ++tx) atomicAdd(&s_win[(ty - r.win.y0) * r.win.w + (tx - r.win.x0)], 1u);
        __builtin_amdgcn_wave_barrier();
        const float inv_w = 1.0f / (float)r.win.w;
#pragma unroll
        for (int j = 0; j < kResvSlots; ++j) {               // ONE global (returning) atomic per touched tile
            const int k = lane + 64 * j;
            const uint32_t c = k < area ? s_win[k] : 0u;
            if (c) r.base[j] = atomicAdd(&tile_count[r.win.tile_of(k, gx, inv_w)], c);
        }
    } else {                                                 // huge footprints: straight to global memory, no slots reserved
        if (lane == 0) atomicOr(&vis_part[kUnresvWord], 1u);  // (the scan reads tile_count2 only if told so)
        if (t.visible)
            for (int ty = t.r1; ty < t.r3; ++ty)
                for (int tx = t.r0; tx < t.r2; ++tx) atomicAdd(&tile_count2[ty * gx + tx], 1u);
    }
    return r;
}
// rec: this wavefront's reservation record.  Every base of the window is written, 0 where the wavefront has no duplicate: the
// scatter reads them all, and so never sees what an earlier frame left in the scratch.
__device__ __forceinline__ void tile_reserve_store(const TileResv &r, uint32_t *__restrict__ rec) {
    const int lane = threadIdx.x & 63;
    if (lane == 0)
        *reinterpret_cast<uint4 *>(rec) = make_uint4((uint32_t)r.win.x0 | ((uint32_t)r.win.y0 << 16), (uint32_t)r.win.w | ((uint32_t)r.win.h << 16), 0u, 0u);
    if (r.win.empty() || !r.win.fits()) return;              // uniform
    const int area = r.win.area();
#pragma unroll
    for (int j = 0; j < kResvSlots; ++j)
        if (lane + 64 * j < area) rec[kResvHdr + lane + 64 * j] = r.base[j];
}

// The per-view tail of both forward kernels: R1 of Gaussian i in view `cam` from what the kernel has in registers (staged: the SH
// colour sum in cj.a0..a2; pre: the covariance row and raw opacity; mean: its means3D row).  WIN: the rectangle is clipped to the window's gx x gy tiles.
template <bool WIN, bool TC = false>
__device__ __forceinline__ PreOut preprocess_view(const d3ga_raster_params &prm, const ViewCam &cam, int i, V3 mean,
                                                    const float *sh_row, bool staged, const ShColJ &cj, bool pre, const float (&pc6)[6],
                                                    float pop, const float *colors_precomp, const float *opacities, const float *scales,
                                                    const float *rotations, const float *cov3D_precomp, int gx, int gy) {
    PreLoaded pl;
    pl.has_sh = staged; pl.has_c6 = pre;
    pl.sh[0] = cj.a0; pl.sh[1] = cj.a1; pl.sh[2] = cj.a2;
#pragma unroll
    for (int k = 0; k < 6; ++k) pl.c6[k] = pc6[k];
    pl.op = pop;
    pl.has_mean = true; pl.mean = mean;
    PreOut o = preprocess_one(prm, cam, i, nullptr, sh_row, colors_precomp, opacities, scales, rotations, cov3D_precomp, pl);
    if constexpr (TC) tile_tighten(o);
    if constexpr (WIN) o = window_clip(o, cam.ox / kTile, cam.oy / kTile, gx, gy);
    return o;
}

// A FULL wavefront of the training forward with full SH rows (M = 16) and precomputed covariances: Gaussian i = this lane's.
// (Covariances from (scale, rotation) take the other order in preprocess_kernel: forming them here was the kernel's register peak.)
// Source order: mean (one load), opacity, covariance row, SH half 0; the projection; the records that the projection alone decides;
// tile histogram and the reservation's returning atomics -- nothing of that depends on SH, and the slab region is free to be the
// tile window until the rows are copied into it (LDS operations of a wavefront execute in order); then the two SH passes, under
// which the atomics return; colour records; reservation record.
// Compiled (ISA, both WIN): mean, opacity and the six loads of half 0 are issued together; vmcnt(7) waits for the mean alone.  The
// COVARIANCE ROW is not among them: the compiler sinks its two loads behind the near-plane test of the projection (the parent had
// them in front of its SH staging), a dependent round trip whose wait, vmcnt(0), also takes in half 0 -- so half 0's latency hides
// under the mean's and the covariance's round trips, not under the projection.  Then projection, eight returning atomics and the
// record stores with nothing waited for, the slab writes of half 0 (vmcnt(10)..(5): the atomics stay out), first pass, half 1.
// Per wavefront: mean | covariance (+ half 0) | half 1, against the parent's mean | half 0 | half 1 | mean again.  slab: its LDS.
template <bool WIN, bool TC = false>
__device__ __forceinline__ void preprocess_full_wavefront(
    const d3ga_raster_params &prm, const ViewCam &cam, const float *__restrict__ means3D, const float *__restrict__ shs,
    const float *__restrict__ opacities, const float *__restrict__ cov3D_precomp, const float *__restrict__ campos, const GeomBuf &geom,
    uint32_t *__restrict__ tile_count,
    uint32_t *__restrict__ tile_count2, uint32_t *__restrict__ vis_part, uint32_t *__restrict__ rec, int32_t *__restrict__ radii,
    int tile_row0, int gx, int gy, float *slab) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int i = blockIdx.x * kBlock + tid;
    const int row0 = i - lane;
    PreLoaded pl;
    pl.has_sh = true; pl.has_c6 = true; pl.has_mean = true;
    pl.mean = ld3(means3D, i);                 // ONE load per Gaussian: the projection and the direction both take the value
    pl.op = opacities[i];
#pragma unroll
    for (int k = 0; k < 6; ++k) pl.c6[k] = cov3D_precomp[6 * (size_t)i + k];
    const int nb = (prm.sh_degree + 1) * (prm.sh_degree + 1);
    float B[16];
    float dx, dy, dz, invd;
    bool visible = false;
    TileResv rs;
    ShColJ cj = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    sh_two_pass48(slab, shs + (size_t)48 * row0, lane, [&]() __attribute__((always_inline)) {
        PreOut o = preprocess_geom(prm, cam, i, pl.mean, opacities, nullptr, nullptr, cov3D_precomp, pl);
        if constexpr (WIN) visible = o.sp.visible;   // before the window clip: what the colour is formed for
        if constexpr (TC) tile_tighten(o);
        if constexpr (WIN) o = window_clip(o, cam.ox / kTile, cam.oy / kTile, gx, gy);
        rs = tile_reserve_issue<true>(reinterpret_cast<uint32_t *>(slab), view_tile_rect(o, tile_row0), gx, tile_count, tile_count2, vis_part);
        invd = write_geom_records_splat(geom, i, o, false, tile_row0, radii);
        sh_view_dir(pl.mean, campos, dx, dy, dz);
        sh_basis(prm.sh_degree, dx, dy, dz, B);
    }, [&](const float *row) __attribute__((always_inline)) {
        cj = sh_accumulate_jacobian(B, dx, dy, dz, row, nb, cj);
    });
    pl.sh[0] = cj.a0; pl.sh[1] = cj.a1; pl.sh[2] = cj.a2;
    float rgb[3] = {0.f, 0.f, 0.f};
    uint8_t clampmask = 0;
    if constexpr (!WIN) visible = invd != 0.f;   // (1 / depth of a visible Gaussian, 0 otherwise: one register less through the passes)
    preprocess_colour(prm, cam, i, pl.mean, nullptr, nullptr, pl, visible, rgb, clampmask);
    write_geom_records_colour(geom, i, rgb[0], rgb[1], rgb[2], invd, clampmask, true, cj);
    tile_reserve_store(rs, rec);
}

// WIN: windowed camera slot (campos: 9 floats, d3ga.h): project with the view's raster size, histogram over the window's tiles
template <bool WANT_J, bool WIN, bool TC = false>      // TC: tile_tighten() in front of the reservation (d3ga_raster_params::tile_cull); WANT_J: a backward will follow (forward_only == 0) and the SH coefficients are staged: leave d(colour)/d(direction) for it
__global__ __launch_bounds__(kBlock) void preprocess_kernel(
    d3ga_raster_params prm, const float *__restrict__ means3D, const float *__restrict__ shs,
    const float *__restrict__ colors_precomp, const float *__restrict__ opacities, const float *__restrict__ scales,
    const float *__restrict__ rotations, const float *__restrict__ cov3D_precomp, const float *__restrict__ viewmatrix,
    const float *__restrict__ projmatrix, const float *__restrict__ campos, GeomBuf geom,
    uint32_t *__restrict__ tile_count, uint32_t *__restrict__ tile_count2, uint32_t *__restrict__ vis_part,
    uint32_t *__restrict__ resv /* this view's reservation records */, int32_t *__restrict__ radii,
    int tile_row0 /* view-batched renders: this view's first tile row in the batch's grid (d3ga.h: n_views); else 0 */) {
    const ViewCam cam = view_cam(prm, viewmatrix, projmatrix, campos, WIN);
    const int gx = (prm.W + kTile - 1) / kTile + (WIN ? 1 : 0), gy = (prm.H + kTile - 1) / kTile + 1;   // (WIN) the window's grid
    // one dynamic LDS region per wavefront, its tile window and its SH staging slab in turn: no workgroup barrier
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *s_sh = reinterpret_cast<float *>(smem);
    const int tid = threadIdx.x, wave = tid >> 6;
    const int i = blockIdx.x * kBlock + tid;
    const int M3 = 3 * prm.M;
    const bool staged = shs != nullptr && sh_staged(prm.M);
    uint32_t *s_win = reinterpret_cast<uint32_t *>(smem) + wave * (staged ? kShHalfSlab : kResvStride);
    uint32_t *const rec = resv + (size_t)(blockIdx.x * (kBlock / 64) + wave) * kResvStride;
    const int row0 = blockIdx.x * kBlock + wave * 64;           // first Gaussian of this wavefront
    // (Training forward with precomputed covariances only.  The forward-only kernel is lighter in its SH passes: carrying the reservation's bases and 1 / depth
    // through them costs it registers, 71 -> 85 VGPRs and from 7 to 5 wavefronts per SIMD.  It keeps the order below.)
    if (WANT_J && staged && cov3D_precomp && M3 == 48 && prm.P - row0 >= 64) {   // wave-uniform: a full wavefront of full rows (M = 16)
        preprocess_full_wavefront<WIN, TC>(prm, cam, means3D, shs, opacities, cov3D_precomp, campos, geom, tile_count, tile_count2, vis_part, rec,
                                           radii, tile_row0, gx, gy, s_sh + wave * kShHalfSlab);
        return;
    }
    // mean (ONE load per Gaussian: the direction and the projection both take the value), covariance row and opacity
    V3 mean = v3(0.f, 0.f, 0.f);
    float pc6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, pop = 0.f;
    const bool pre = staged && cov3D_precomp != nullptr;
    if (i < prm.P) {
        mean = ld3(means3D, i);
        if (pre) {
#pragma unroll
            for (int k = 0; k < 6; ++k) pc6[k] = cov3D_precomp[6 * (size_t)i + k];
            pop = opacities[i];
        }
    }
    ShColJ cj = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float acc[3] = {0.f, 0.f, 0.f};
    // every other wavefront (partial, M != 16, unstaged colours): colour first, then the projection and the reservation
    if (staged) {
        staged_sh_colour<WANT_J>(prm, mean, shs, campos, s_sh, acc, cj);
        if (!WANT_J) { cj.a0 = acc[0]; cj.a1 = acc[1]; cj.a2 = acc[2]; }
    }
    TileRect tr = {false, 0, 0, 0, 0};
    PreOut o = {};
    if (i < prm.P) {
        // two call sites so that each inlined copy sees ONE address space (registers vs global_load, never flat)
        o = staged ? preprocess_view<WIN, TC>(prm, cam, i, mean, nullptr, true, cj, pre, pc6, pop, colors_precomp, opacities, scales,
                                              rotations, cov3D_precomp, gx, gy)
                   : preprocess_view<WIN, TC>(prm, cam, i, mean, shs ? shs + (size_t)M3 * i : nullptr, false, cj, false, pc6, pop,
                                              colors_precomp, opacities, scales, rotations, cov3D_precomp, gx, gy);
        tr = view_tile_rect(o, tile_row0);
    }
    // the slab is dead now; the reservation's atomics are in flight while the records are stored
    const TileResv rs = tile_reserve_issue(s_win, tr, gx, tile_count, tile_count2, vis_part);
    if (i < prm.P) write_geom_records(geom, i, o, !cov3D_precomp, tile_row0, radii, WANT_J, cj);
    tile_reserve_store(rs, rec);
}

// The same for KV views of ONE set of Gaussians in one pass (view-batched renders with shared geometry, d3ga.h: n_views): the
// Gaussian's mean, covariance, opacity and -- the bulk of the kernel's traffic, 12 M bytes -- its SH row are read ONCE; per view the
// colour (and its direction Jacobian) is formed from the staged row with that view's direction, the projection runs, the records go
// to the view's section of the batch's buffers and the view's histogram pass follows.  Per view the arithmetic is that of
// preprocess_kernel (same inlined functions, same order): bit-identical records.  views: KV cameras starting at `view0`.
// Unlike staged_sh_colour, the basis is formed inside the passes: the registers cannot hold KV of them.
template <bool WANT_J, int KV>
__device__ __forceinline__ void staged_sh_colour_views(const d3ga_raster_params &prm, const float *__restrict__ means3D, size_t pv,
                                                       const float *__restrict__ shs, const ViewCams<KV> &cams, float *s_sh,
                                                       ShColJ (&cj)[KV]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x * kBlock + tid;
    const int M3 = 3 * prm.M;
    float *slab = s_sh + wave * kShHalfSlab;
    const int row0 = blockIdx.x * kBlock + wave * 64;
    const int rows = min(64, prm.P - row0);
    const int nb = (prm.sh_degree + 1) * (prm.sh_degree + 1);
    auto eval = [&](const float *row) __attribute__((always_inline)) {
#pragma unroll
        for (int v = 0; v < KV; ++v) {
            float B[16];
            const float *mv = means3D + 3 * pv * v;                  // (a batch of frames: every view's own means)
            if (WANT_J) {
                float dx, dy, dz;
                sh_view_dir(mv, i, cams.cp[v], dx, dy, dz);
                sh_basis(prm.sh_degree, dx, dy, dz, B);
                cj[v] = sh_accumulate_jacobian(B, dx, dy, dz, row, nb, cj[v]);
            } else {
                sh_view_basis(prm, mv, i, cams.cp[v], B);
                float acc[3] = {cj[v].a0, cj[v].a1, cj[v].a2};
                sh_accumulate(B, row, 0, 16, nb, acc);
                cj[v].a0 = acc[0]; cj[v].a1 = acc[1]; cj[v].a2 = acc[2];
            }
        }
    };
    if (M3 == 48 && rows == 64) {                              // wave-uniform: a full wavefront of full rows
        const float *src = shs + (size_t)48 * row0;
        const ShRegs<kShPassRows> h0 = sh_rows48_load<kShPassRows>(src, lane);
        const ShRegs<kShPassRows> h1 = sh_rows48_load<kShPassRows>(src + 48 * kShPassRows, lane);
        __builtin_amdgcn_wave_barrier();
        sh_rows48_to_slab<kShPassRows>(slab, h0, lane);
        __builtin_amdgcn_wave_barrier();
        if (lane / kShPassRows == 0) eval(slab + (lane % kShPassRows) * kShRow);
        __builtin_amdgcn_wave_barrier();
        sh_rows48_to_slab<kShPassRows>(slab, h1, lane);
        __builtin_amdgcn_wave_barrier();
        if (lane / kShPassRows == 1) eval(slab + (lane % kShPassRows) * kShRow);
        return;
    }
    for (int h = 0; h < 2; ++h) {
        const int r = min(kShPassRows, rows - kShPassRows * h);
        __builtin_amdgcn_wave_barrier();
        if (r > 0) sh_slab_load(slab, shs + (size_t)M3 * (row0 + kShPassRows * h), r, M3, lane);
        __builtin_amdgcn_wave_barrier();
        if (i < prm.P && lane / kShPassRows == h) eval(slab + (lane % kShPassRows) * kShRow);
    }
}

template <bool WANT_J, int KV, bool TC = false>
__global__ __launch_bounds__(kBlock) void preprocess_views_kernel(
    d3ga_raster_params prm, const float *__restrict__ means3D, const float *__restrict__ shs,
    const float *__restrict__ colors_precomp, const float *__restrict__ opacities, const float *__restrict__ scales,
    const float *__restrict__ rotations, const float *__restrict__ cov3D_precomp, ViewCams<KV> cams, GeomBuf geom /* of the first view */,
    uint32_t *__restrict__ tile_count, uint32_t *__restrict__ tile_count2, uint32_t *__restrict__ vis_part,
    uint32_t *__restrict__ resv /* reservation records of the first view */, int32_t *__restrict__ radii /* of the first view */,
    int tile_row0, int gyv, size_t pv /* records between the views' geometry: 0 = k cameras of one set of Gaussians, P = a batch of frames */) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *s_sh = reinterpret_cast<float *>(smem);
    const int tid = threadIdx.x, wave = tid >> 6;
    const int i = blockIdx.x * kBlock + tid;
    uint32_t *s_win = reinterpret_cast<uint32_t *>(smem) + wave * kShHalfSlab;      // the wavefront's slab, once the colours are formed
    const size_t wpv = (size_t)gridDim.x * (kBlock / 64);                            // reservation records per view (resv_waves)
    // shared by the views: covariance row and opacity (in flight while the SH rows are staged)
    float pc6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, pop = 0.f;
    const bool pre = cov3D_precomp != nullptr && pv == 0;
    if (pre && i < prm.P) {
#pragma unroll
        for (int k = 0; k < 6; ++k) pc6[k] = cov3D_precomp[6 * (size_t)i + k];
        pop = opacities[i];
    }
    ShColJ cj[KV];
#pragma unroll
    for (int v = 0; v < KV; ++v) cj[v] = ShColJ{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    staged_sh_colour_views<WANT_J, KV>(prm, means3D, pv, shs, cams, s_sh, cj);
    const int gx = (prm.W + kTile - 1) / kTile;
#pragma unroll
    for (int v = 0; v < KV; ++v) {                              // (the window is the wavefront's own: slab -> window -> window in program order)
        TileRect tr = {false, 0, 0, 0, 0};
        PreOut o = {};
        if (i < prm.P) {
            const size_t og = pv * v;
            o = preprocess_view<false, TC>(prm, view_cam(prm, cams.vm[v], cams.pm[v], cams.cp[v], false), i, ld3(means3D + 3 * og, i), nullptr, true,
                                           cj[v], pre, pc6, pop, colors_precomp, opacities, scales ? scales + 3 * og : nullptr,
                                           rotations ? rotations + 4 * og : nullptr, cov3D_precomp ? cov3D_precomp + 6 * og : nullptr, gx, 0);
            tr = view_tile_rect(o, tile_row0 + v * gyv);
        }
        const TileResv rs = tile_reserve_issue(s_win, tr, gx, tile_count, tile_count2, vis_part);
        if (i < prm.P)
            write_geom_records(geom_view(geom, prm.P, v), i, o, !cov3D_precomp, tile_row0 + v * gyv, radii + (size_t)prm.P * v, WANT_J, cj[v]);
        tile_reserve_store(rs, resv + (wpv * v + blockIdx.x * (kBlock / 64) + wave) * kResvStride);
    }
}

// Second render of the SAME geometry with other colours (the reference's training step renders RGB and a silhouette
// pass from one garment_pkg, models/trainer.py:102-110): copies the geometry records of `src` to `dst` and evaluates
// only the colour (SH of this camera or colors_precomp) -- the projection, the tile histogram and the whole binning
// stage of the second pass disappear; `dst` then shares the first pass's binning buffer.
template <bool WANT_J>
__global__ __launch_bounds__(kBlock) void recolor_kernel(d3ga_raster_params prm, const float *__restrict__ means3D,
                                                         const float *__restrict__ shs,
                                                         const float *__restrict__ colors_precomp,
                                                         const float *__restrict__ campos, GeomBuf src, GeomBuf dst) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *s_sh = reinterpret_cast<float *>(smem);
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const int M3 = 3 * prm.M;
    const bool staged = shs != nullptr && sh_staged(prm.M);
    ShColJ cj = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float acc[3] = {0.f, 0.f, 0.f};
    if (staged) staged_sh_colour<WANT_J>(prm, i < prm.P ? ld3(means3D, i) : v3(0.f, 0.f, 0.f), shs, campos, s_sh, acc, cj);
    if (i >= prm.P) return;
    if (WANT_J) {
        acc[0] = cj.a0; acc[1] = cj.a1; acc[2] = cj.a2;
        dcol_store(dst.dcol, dst.dcol_stride, i, cj);
    }
    const uint2 rc = src.rect[i];
    const bool visible = rect_visible(rc.x, rc.y);
    const float depth = src.depth[i];
    dst.depth[i] = depth;
    dst.conic_o[i] = src.conic_o[i];
    dst.xyh[i] = src.xyh[i];
    dst.rect[i] = rc;
#pragma unroll
    for (int k = 0; k < 6; ++k) dst.cov3D[6 * (size_t)i + k] = src.cov3D[6 * (size_t)i + k];
    float rgb[3] = {0.f, 0.f, 0.f};
    uint8_t mask = 0;
    if (visible) {
        if (colors_precomp) {
            rgb[0] = colors_precomp[3 * (size_t)i]; rgb[1] = colors_precomp[3 * (size_t)i + 1];
            rgb[2] = colors_precomp[3 * (size_t)i + 2];
        } else {
            if (!staged) {
                float B[16];
                sh_view_basis(prm, means3D, i, campos, B);
                sh_accumulate(B, shs + (size_t)M3 * i, 0, 16, (prm.sh_degree + 1) * (prm.sh_degree + 1), acc);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float v = acc[c] + 0.5f;
                if (v < 0.f) mask |= (uint8_t)(1u << c);
                rgb[c] = fmaxf(v, 0.f);
            }
        }
    }
    dst.rgb_invd[i] = make_float4(rgb[0], rgb[1], rgb[2], visible ? 1.0f / depth : 0.f);
    dst.clamped[i] = mask;
}

// the records of a view's backward as the per-view bodies read them (raster_pre_body.h)
__device__ __forceinline__ ViewRecs view_recs(const GeomBuf &g, const float *acc) {
    return ViewRecs{reinterpret_cast<const uint32_t *>(g.rect), acc, g.clamped, reinterpret_cast<const float *>(g.conic_o), g.dcol,
                    g.dcol_stride};
}

// What preprocess_bwd_kernel<., true> takes behind its own arguments: the deform backward's inputs and outputs (d3ga.h:
// d3ga_cage_deform_in / _grads / _route, as cage_deform_bwd_kernel takes them).
template <bool GEO>      // GEO: dL/dmean and dL/dcov are written as well (both arrays given)
struct DeformTailT {
    static constexpr bool kGeo = GEO;
    const float *tetpoints;
    const int32_t *tetras, *tetra_id;
    const float *barys, *canon_grad, *scales, *rots, *delta_barys;
    int flags;
    float *g_barys, *g_scales, *g_rots, *corner_grads;
    DeformMerge mg;
};
using DeformTail = DeformTailT<false>;
using DeformTailGeo = DeformTailT<true>;
static_assert(kMergeBlock == kBlock, "the block merge is laid out for the workgroup size");
static_assert(sizeof(float) * 3 * kMergeItems <= kShLdsBytes, "the merge planes take the place of the SH slabs");
template <class T>
__device__ __forceinline__ const T &first_of(const T &t) { return t; }

// DEFORM (single view, precomputed covariance produced by the cage deformation; d3ga_raster_preprocess_bwd_deform): the thread
// keeps dL/dmean and dL/dcov of its Gaussian in registers and runs the deform backward on them -- what cage_deform_bwd_kernel
// would read back from memory in the next launch -- from the DeformTail `tail` behind the arguments.  The two arrays are written
// only where their pointers are given: both or neither, and given (DeformTailT<true>, an instantiation of its own) the thread
// writes them through the plain kernel's own calls and goes on from the values written -- every output is then the two-kernel
// path's bit for bit, where the register variant differs in the last bit of dL/dmean (the compiler contracts its multiply-adds
// differently; docs/LOG.md).  Source order: the dependent chain tetra_id -> tetras -> tetpoints is issued with the record
// loads; the streaming deform inputs are loaded behind the SH phase, so the register peak is the larger of the two phases;
// the merge planes reuse the SH slabs' LDS once every wavefront has read its slab (one workgroup barrier more than the merge's
// own).  Every thread reaches both barriers: i >= P and culled Gaussians go through with zero gradients.
template <bool WIN, bool DEFORM = false, class... TAIL>      // WIN: windowed camera slot -- the view's raster size from its camera row
__global__ __launch_bounds__(kBlock) void preprocess_bwd_kernel(
    d3ga_raster_params prm, const float *__restrict__ means3D, const float *__restrict__ shs,
    const float *__restrict__ scales, const float *__restrict__ rotations, const float *__restrict__ viewmatrix,
    const float *__restrict__ projmatrix, const float *__restrict__ campos, GeomBuf geom,
    const float *__restrict__ acc, float *__restrict__ dL_dmeans3D, float *__restrict__ dL_dmeans2D,
    float *__restrict__ dL_dopacity, float *__restrict__ dL_dsh, float *__restrict__ dL_dcolors,
    float *__restrict__ dL_dcov3D, float *__restrict__ dL_dscales, float *__restrict__ dL_drots,
    const float *__restrict__ cov3D_precomp, int accum /* views > 0 of a batch: add to the gradients of inputs the views share (raster_pre_body.h) */,
    TAIL... tail) {
    const ViewCam cam = view_cam(prm, viewmatrix, projmatrix, campos, WIN);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *s_sh = reinterpret_cast<float *>(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x * kBlock + tid;
    const int M3 = 3 * prm.M;
    const bool staged = shs != nullptr && sh_staged(prm.M);      // dL_dsh may be null (factored SH gradient)
    const int row0 = blockIdx.x * kBlock + wave * 64;
    const int rows = min(64, prm.P - row0);
    float *slab = s_sh + wave * kShSlab;
    const bool full48 = M3 == 48 && rows == 64;                 // wave-uniform
    // This Gaussian's records first, unconditionally (an invisible one has an all-zero accumulator row and a valid
    // covariance row): they are in flight together with the SH rows instead of two dependent round trips behind them.
    uint2 rc = make_uint2(0u, 0u);
    AccRec ar;                                                  // (set for i < P only, as a[] was: zero-initialising it changes the packed float code)
    float c6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    uint8_t clampmask = 0;
    float act_opacity = 0.f;
    if (i < prm.P) {
        rc = geom.rect[i];
        ar = acc_load(acc, i, prm.acc_self_clearing);
#pragma unroll
        for (int k = 0; k < 6; ++k) c6[k] = (cov3D_precomp ? cov3D_precomp : geom.cov3D)[6 * (size_t)i + k];   // (the forward kept no copy of a precomputed one)
        clampmask = geom.clamped[i];
        act_opacity = geom.conic_o[i].w;
    }
    // (DEFORM) the tail's dependent chain, three round trips deep, in flight with the records: this Gaussian's tet and its corners
    DeformIn din;
    int tet = 0;
    if constexpr (DEFORM) {
        const auto &dt = first_of(tail...);
        din.x0 = din.x1 = din.x2 = din.x3 = v3(0.f, 0.f, 0.f);
        int4 vid;
        if (i < prm.P) tet = load_deform_corners(i, dt.tetpoints, dt.tetras, dt.tetra_id, din, vid);
    }
    float g9[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // (DEFORM) dL/dmean, dL/dcov of this Gaussian
    // Round 5: the forward left d(colour)/d(direction) of every Gaussian (geom.dcol, 36 bytes) when it staged the coefficients and
    // a backward was to follow: the coefficients themselves (192 bytes per Gaussian) are then not read here at all -- the slab
    // only collects the gradient rows for the coalesced store.
    const bool have_j = staged && !prm.forward_only;
    ShColJ jd = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (have_j && i < prm.P) jd = dcol_load(geom.dcol, geom.dcol_stride, i);
    if (staged && !have_j) {
        if (full48) sh_rows48_to_slab<64>(slab, sh_rows48_load<64>(shs + (size_t)48 * row0, lane), lane);
        else if (rows > 0) sh_slab_load(slab, shs + (size_t)M3 * row0, rows, M3, lane);
        __builtin_amdgcn_wave_barrier();          // the slab is private to the wavefront: program order suffices
    }
    if (i < prm.P) {
        const bool visible = rect_visible(rc.x, rc.y);
        if (!visible) {
#pragma unroll
            for (int k = 0; k < 12; ++k) ar.a[k] = 0.f;
#pragma unroll
            for (int k = 0; k < 6; ++k) c6[k] = 0.f;
            act_opacity = 0.f;
        }
        // two call sites so that each inlined copy sees ONE address space (LDS row vs global row, never flat);
        // staged: the gradient row overwrites the coefficient row in place
        if constexpr (DEFORM) {
            if constexpr (std::decay_t<decltype(first_of(tail...))>::kGeo) {
                // the two arrays are wanted as well: written as the plain kernel writes them, by the same calls, and taken from there
                if (staged)
                    preprocess_bwd_one(prm, cam, i, visible, means3D, slab + lane * kShRow, scales, rotations, c6, clampmask, ar.a,
                                       dL_dmeans3D, dL_dmeans2D, dL_dopacity, dL_dsh ? slab + lane * kShRow : nullptr, dL_dcolors,
                                       dL_dcov3D, dL_dscales, dL_drots, act_opacity, have_j, jd, accum);
                else
                    preprocess_bwd_one(prm, cam, i, visible, means3D, shs ? shs + (size_t)M3 * i : nullptr, scales, rotations, c6,
                                       clampmask, ar.a, dL_dmeans3D, dL_dmeans2D, dL_dopacity, dL_dsh ? dL_dsh + (size_t)M3 * i : nullptr,
                                       dL_dcolors, dL_dcov3D, dL_dscales, dL_drots, act_opacity, false, ShColJ(), accum);
#pragma unroll
                for (int k = 0; k < 3; ++k) g9[k] = dL_dmeans3D[3 * (size_t)i + k];
#pragma unroll
                for (int k = 0; k < 6; ++k) g9[3 + k] = dL_dcov3D[6 * (size_t)i + k];
            } else {
                // preprocess_bwd_one itself, as Gaussian 0 of arrays that begin at this Gaussian's rows, with g9 as its dL/dmean
                // and dL/dcov arrays: the nine values stay in registers
                const size_t u = (size_t)i;
                float *const m2d = dL_dmeans2D ? dL_dmeans2D + 3 * u : nullptr, *const dop = dL_dopacity ? dL_dopacity + u : nullptr;
                float *const dcl = dL_dcolors ? dL_dcolors + 3 * u : nullptr;
                if (staged)
                    preprocess_bwd_one(prm, cam, 0, visible, means3D + 3 * u, slab + lane * kShRow, nullptr, nullptr, c6, clampmask, ar.a,
                                       g9, m2d, dop, dL_dsh ? slab + lane * kShRow : nullptr, dcl, g9 + 3, nullptr, nullptr, act_opacity,
                                       have_j, jd, 0);
                else
                    preprocess_bwd_one(prm, cam, 0, visible, means3D + 3 * u, shs ? shs + (size_t)M3 * i : nullptr, nullptr, nullptr, c6,
                                       clampmask, ar.a, g9, m2d, dop, dL_dsh ? dL_dsh + (size_t)M3 * i : nullptr, dcl, g9 + 3, nullptr,
                                       nullptr, act_opacity, false, ShColJ(), 0);
            }
        } else if (staged)
            preprocess_bwd_one(prm, cam, i, visible, means3D, slab + lane * kShRow, scales, rotations, c6, clampmask, ar.a, dL_dmeans3D,
                               dL_dmeans2D, dL_dopacity, dL_dsh ? slab + lane * kShRow : nullptr, dL_dcolors, dL_dcov3D, dL_dscales,
                               dL_drots, act_opacity, have_j, jd, accum);
        else
            preprocess_bwd_one(prm, cam, i, visible, means3D, shs ? shs + (size_t)M3 * i : nullptr, scales, rotations, c6, clampmask,
                               ar.a, dL_dmeans3D, dL_dmeans2D, dL_dopacity, dL_dsh ? dL_dsh + (size_t)M3 * i : nullptr, dL_dcolors,
                               dL_dcov3D, dL_dscales, dL_drots, act_opacity, false, ShColJ(), accum);
    }
    if (staged && dL_dsh) {
        __builtin_amdgcn_wave_barrier();          // the slab is private to the wavefront: program order suffices
        if (full48) sh_rows48_store<64>(slab, dL_dsh + (size_t)48 * row0, lane);
        else if (rows > 0) sh_slab_store(slab, dL_dsh + (size_t)M3 * row0, rows, M3, lane);
    }
    if constexpr (DEFORM) {
        const auto &dt = first_of(tail...);
        DeformGrad o;
        if (i < prm.P) {
            load_deform_streams(i, tet, dt.barys, dt.canon_grad, dt.scales, dt.rots, dt.delta_barys, dt.flags, din);
            deform_bwd(din, g9, g9 + 3, o);
            store_deform_grads(i, dt.flags, din, o, dt.g_barys, dt.g_scales, dt.g_rots);
        }
        if (dt.mg.item_pos) {
            __syncthreads();                      // every wavefront has read its slab: the merge planes take the slabs' place
            deform_merge_epilogue(*reinterpret_cast<float (*)[3][kMergeItems]>(smem), dt.mg, prm.P, i, i < prm.P, o);
        } else if (dt.corner_grads && i < prm.P) {
            store_corner_records(dt.corner_grads, i, o);
        }
    }
}

// R6 for the views of a batch that share their geometry (d3ga.h: n_views without per_view_geometry), ONE pass: thread i walks the kv
// views of Gaussian i (preprocess_bwd_views_one), sums the gradients of the shared inputs in registers and writes every output ONCE:
// no read-modify-write of dL/dmeans3D / dL/dcov / dL/dopacity per view, no (P,3) factors through memory, the (P,M,3) SH row formed
// there (sum_v Y(dir_v) (x) g_v, as sh_grad_from_views_kernel forms it) instead of by a pass of its own.  SH colours need the
// forward's dcol planes (staged coefficients, forward_only == 0): the launcher falls back to per-view launches otherwise, and for the
// factored SH output of the camera-sharded exchange.  accum: a later group of a batch of more than kMaxGroup views -- every output is
// added to, except the per-view ones.  pva (d3ga.h: per_view_appearance, precomputed colours): dL/dopacity and dL/dcolour are
// written per view at record v P + i of the group, not summed.
constexpr int kMaxGroup = 8;
template <bool WIN>      // WIN: windowed camera slots -- every view's raster size from its camera row
__global__ __launch_bounds__(kBlock) void preprocess_bwd_views_kernel(
    d3ga_raster_params prm, int kv, const float *__restrict__ means3D, bool sh_path, const float *__restrict__ scales,
    const float *__restrict__ rotations, const float *__restrict__ cov3D_precomp, ViewCams<kMaxGroup> cams, GeomBuf geom /* first view of the group */,
    const float *__restrict__ acc /* first view of the group */, float *__restrict__ dL_dmeans3D, float *__restrict__ dL_dmeans2D /* first view | null */,
    float *__restrict__ dL_dopacity, float *__restrict__ dL_dsh, float *__restrict__ dL_dcolors, float *__restrict__ dL_dcov3D,
    float *__restrict__ dL_dscales, float *__restrict__ dL_drots, bool accum,
    size_t pv /* records between the views' geometry AND geometry gradients: 0 = shared (summed), P = a batch of frames (written per view) */,
    bool pva /* per-view appearance: dL_dopacity / dL_dcolors are (kv,P) / (kv,P,3) of the group's first view */) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *s_sh = reinterpret_cast<float *>(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x * kBlock + tid;
    const int M3 = 3 * prm.M;
    const int row0 = blockIdx.x * kBlock + wave * 64;
    const int rows = min(64, prm.P - row0);
    float *slab = s_sh + wave * kShSlab;
    if (i < prm.P)
        preprocess_bwd_views_one(prm, i, kv, WIN, cams, view_recs(geom, acc), means3D, cov3D_precomp ? cov3D_precomp : geom.cov3D,
                                 scales, rotations, sh_path, pv, pva, accum, dL_dmeans3D, dL_dmeans2D, dL_dopacity, dL_dcolors,
                                 dL_dcov3D, dL_dscales, dL_drots, sh_path && dL_dsh ? slab + lane * kShRow : nullptr);
    if (sh_path && dL_dsh) {
        __builtin_amdgcn_wave_barrier();          // the slab is private to the wavefront: program order suffices
        if (accum) {                              // a later group of a large batch: add to what the earlier groups wrote
            const int nvec = rows > 0 ? rows * M3 / 4 : 0;
            float4 *dst = reinterpret_cast<float4 *>(dL_dsh + (size_t)M3 * row0);
            for (int v = lane; v < nvec; v += 64) {
                const int e = 4 * v, r = e / M3, c = e - r * M3;
                const float4 x = *reinterpret_cast<const float4 *>(slab + r * kShRow + c);
                float4 y = dst[v];
                y.x += x.x; y.y += x.y; y.z += x.z; y.w += x.w;
                dst[v] = y;
            }
        } else if (M3 == 48 && rows == 64) sh_rows48_store<64>(slab, dL_dsh + (size_t)48 * row0, lane);
        else if (rows > 0) sh_slab_store(slab, dL_dsh + (size_t)M3 * row0, rows, M3, lane);
    }
}

// View-sharded training: the SH gradient of one view is rank-1 per Gaussian,
//   dL/dsh[i][k][c] = basis_k(normalize(mean_i - campos_v)) * g_v[i][c],      g_v = clamp-masked dL/dcolour,
// so the ranks exchange the (P,3) factor g_v (all-gather) instead of summing (P,M,3) blocks (all-reduce) and every rank
// rebuilds   dL_dsh = scale * sum_v basis(dir_v) (x) g_v   here.  One thread per Gaussian, 48 accumulators in
// registers, rows leave through the per-wavefront LDS slab (16 B/lane contiguous stores).
__global__ __launch_bounds__(kBlock) void sh_grad_from_views_kernel(
    int P, int M, int sh_degree, int n_views, const float *__restrict__ means3D, int64_t means_stride /* floats between the views' means (0: shared) */,
    const float *__restrict__ g_views, int64_t g_stride, const float *__restrict__ campos_views, int64_t campos_stride, float scale,
    float *__restrict__ dL_dsh) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *s_sh = reinterpret_cast<float *>(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x * kBlock + tid;
    const int M3 = 3 * M;
    const bool staged = sh_staged(M);
    const int row0 = blockIdx.x * kBlock + wave * 64;
    const int rows = min(64, P - row0);
    float *slab = s_sh + wave * kShSlab;
    if (i < P) {
        float out[48];
#pragma unroll
        for (int k = 0; k < 48; ++k) out[k] = 0.f;
        const int nb = (sh_degree + 1) * (sh_degree + 1);
        for (int v = 0; v < n_views; ++v) {
            const float *g = g_views + v * g_stride + 3 * (size_t)i;
            const float g0 = g[0], g1 = g[1], g2 = g[2];
            if (g0 == 0.f && g1 == 0.f && g2 == 0.f) continue;        // culled / invisible / clamped in this view
            const V3 mean = ld3(means3D + v * means_stride, i);
            const float *cp = campos_views + v * campos_stride;
            const V3 d0 = mean - v3(cp[0], cp[1], cp[2]);
            const float inv = 1.0f / sqrtf(dot(d0, d0));
            float B[16];
            sh_basis(sh_degree, d0.x * inv, d0.y * inv, d0.z * inv, B);
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (k < nb) {
                    out[3 * k] += B[k] * g0; out[3 * k + 1] += B[k] * g1; out[3 * k + 2] += B[k] * g2;
                }
        }
        float *row = staged ? slab + lane * kShRow : nullptr;
#pragma unroll
        for (int k = 0; k < 48; ++k)
            if (k < M3) {
                if (staged) row[k] = out[k] * scale;
                else dL_dsh[(size_t)M3 * i + k] = out[k] * scale;
            }
    }
    if (staged) {
        __syncthreads();
        if (rows > 0) sh_slab_store(slab, dL_dsh + (size_t)M3 * row0, rows, M3, lane);
    }
}

__global__ __launch_bounds__(kBlock) void mark_visible_kernel(int P, const float *__restrict__ means3D,
                                                              const float *__restrict__ viewmatrix,
                                                              uint8_t *__restrict__ visible) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P) return;
    visible[i] = xform_point(viewmatrix, ld3(means3D, i)).z > kNear ? 1 : 0;
}

}  // namespace d3ga

using namespace d3ga;

static int validate(const d3ga_raster_params *prm) {
    if (!prm) return D3GA_E_NULL;
    if (prm->P < 0 || prm->W <= 0 || prm->H <= 0 || prm->M < 0 || prm->M > 16) return D3GA_E_SIZE;
    if (prm->sh_degree < 0 || prm->sh_degree > 3) return D3GA_E_CONFIG;
    if (prm->n_views < 0) return D3GA_E_SIZE;
    if (grid_x(prm) > 65535 || (int64_t)grid_y(prm) * n_views_of(prm) > 65535) return D3GA_E_SIZE;
    if ((int64_t)prm->P * n_views_of(prm) >= (1ll << 31)) return D3GA_E_SIZE;
    return D3GA_OK;
}

// The launchers' shared rules.  staged: the kernels move the SH rows through the LDS slabs; leaves_dcol: the forward then leaves
// GeomBuf::dcol for a backward to follow, and the backward reads it instead of the coefficients.
static bool staged(const d3ga_raster_params *prm, const float *shs) { return shs != nullptr && sh_staged(prm->M); }
static bool leaves_dcol(const d3ga_raster_params *prm, const float *shs) { return staged(prm, shs) && !prm->forward_only; }
// dynamic LDS of a launch: the SH slabs if staged, at least `floor` bytes (the forward's tile window)
static size_t lds_bytes(bool staged, size_t slabs, size_t floor = 0) { return staged && slabs > floor ? slabs : floor; }
// floats per camera row (d3ga.h: camera slots carry the two tangents behind the position, windowed ones also the raster and window)
static int cam_stride(const d3ga_raster_params *prm) {
    return prm->tanfovx > 0.f ? 3 : (is_windowed(prm) ? D3GA_CAMERA_SLOT_WINDOWED_FLOATS : 5);
}
// the cameras of views [v0, v0 + kv) (slots past kv repeat view v0)
template <int K>
static ViewCams<K> view_cams(const float *vm, const float *pm, const float *cp, int stride, int v0, int kv) {
    ViewCams<K> c;
    for (int q = 0; q < K; ++q) {
        const int v = v0 + (q < kv ? q : 0);
        c.vm[q] = vm + 16 * (size_t)v; c.pm[q] = pm + 16 * (size_t)v; c.cp[q] = cp + (size_t)stride * v;
    }
    return c;
}
// a per-record array of a batch at record r (n floats per record), or null
template <class T>
static T *at(T *p, size_t n, size_t r) { return p ? p + n * r : nullptr; }

extern "C" int d3ga_raster_preprocess(const d3ga_raster_params *prm, const float *means3D, const float *shs,
                                      const float *colors_precomp, const float *opacities, const float *scales,
                                      const float *rotations, const float *cov3D_precomp, const float *viewmatrix,
                                      const float *projmatrix, const float *campos, void *geom, void *binning,
                                      int64_t d_capacity, int32_t *radii, d3ga_stream_t stream) {
    D3GA_TRY(validate(prm));
    if (!geom || !binning || !viewmatrix || !projmatrix || !campos) return D3GA_E_NULL;
    if (d_capacity < 0) return D3GA_E_SIZE;
    hipStream_t s = (hipStream_t)stream;
    const int views = n_views_of(prm), gyv = grid_y(prm);
    const int64_t tiles = (int64_t)grid_x(prm) * gyv * views;
    const bool wnd = is_windowed(prm);
    BinBuf bin = carve_bin(binning, tiles, d_capacity);
    // counters + tile_count + tile_count2 + vis_part are adjacent: one clear
    D3GA_HIP(zero_async(bin.counters, 256 + 2 * align256(4 * tiles) + 4 * kVisParts * kVisStride, s));
    if (wnd) hipLaunchKernelGGL(window_table_kernel, dim3((views + 63) / 64), dim3(64), 0, s, *prm, campos, views, win_table(binning, tiles, d_capacity));
    if (prm->P == 0) return D3GA_OK;          // empty scene: every per-Gaussian tensor is empty (NULL)
    if ((shs != nullptr) == (colors_precomp != nullptr)) return D3GA_E_CONFIG;
    const bool pva = views > 1 && prm->per_view_appearance;   // (k,P) opacities and (k,P,3) colours: precomputed colours only (d3ga.h)
    if (pva && shs) return D3GA_E_CONFIG;
    const bool sr = scales != nullptr && rotations != nullptr;
    if (sr == (cov3D_precomp != nullptr)) return D3GA_E_CONFIG;
    if (shs && (prm->sh_degree + 1) * (prm->sh_degree + 1) > prm->M) return D3GA_E_CONFIG;
    if (!means3D || !opacities || !radii) return D3GA_E_NULL;
    const GeomBuf g = carve_geom(geom, (int64_t)prm->P * views);
    const size_t lds = lds_bytes(staged(prm, shs), kShHalfLdsBytes, (size_t)(kBlock / 64) * kResvStride * 4);
    uint32_t *const resv = resv_records(binning, tiles, d_capacity, views, wnd);
    const size_t resv_view = (size_t)resv_waves(prm->P) * kResvStride;                 // words between the views' records
    const bool want_j = leaves_dcol(prm, shs);
    const bool tc = prm->tile_cull != 0;      // the instantiations that bin by the alpha >= 1/255 box (tile_tighten)
    const int cs = cam_stride(prm);
    // a batch of views writes view v's records at v P + i of the batch's buffers: grouped launches below when the SH row can be
    // shared, else one launch per view (a streaming kernel at the copy rate gains nothing from a taller grid)
    const size_t pv = (views > 1 && prm->per_view_geometry) ? (size_t)prm->P : 0;      // records between the views' geometry (0: shared)
    const size_t pa = pva ? (size_t)prm->P : 0;                                        // ... and between their opacities / colours
    const dim3 grid((prm->P + kBlock - 1) / kBlock), block(kBlock);
    int v0 = 0;
    // k cameras of ONE set of Gaussians with staged SH colours: groups of up to four views per pass (preprocess_views_kernel: the
    // 12 M-byte coefficient row, the mean and the covariance are read once per group instead of once per view).  SH only, so never
    // with per-view appearance (refused above): the group kernel reads one opacity per Gaussian for all its views
    const bool grouped = views > 1 && !pva && !wnd && staged(prm, shs);
    auto launch_group = [&](auto kv) {        // views [v0, v0 + KV)
        constexpr int KV = decltype(kv)::value;
        const size_t og = pv * v0;
        const auto kernel = tc ? (want_j ? preprocess_views_kernel<true, KV, true> : preprocess_views_kernel<false, KV, true>)
                               : (want_j ? preprocess_views_kernel<true, KV> : preprocess_views_kernel<false, KV>);
        hipLaunchKernelGGL(kernel, grid, block, lds, s, *prm,
                           at(means3D, 3, og), shs, colors_precomp, opacities, at(scales, 3, og), at(rotations, 4, og),
                           at(cov3D_precomp, 6, og), view_cams<KV>(viewmatrix, projmatrix, campos, cs, v0, KV), geom_view(g, prm->P, v0),
                           bin.tile_count, bin.tile_count2, bin.vis_part, resv + resv_view * v0, radii + (size_t)prm->P * v0, v0 * gyv,
                           gyv, pv);
        v0 += KV;
    };
    while (grouped && views - v0 >= 2) {
        const int left = views - v0;
        if (left >= 4 && left != 5) launch_group(std::integral_constant<int, 4>());     // (5 = 3 + 2: no single view left over)
        else if (left == 3 || left == 5) launch_group(std::integral_constant<int, 3>());
        else launch_group(std::integral_constant<int, 2>());
    }
    const auto kernel = tc ? (want_j ? (wnd ? preprocess_kernel<true, true, true> : preprocess_kernel<true, false, true>)
                                      : (wnd ? preprocess_kernel<false, true, true> : preprocess_kernel<false, false, true>))
                            : (want_j ? (wnd ? preprocess_kernel<true, true> : preprocess_kernel<true, false>)
                                      : (wnd ? preprocess_kernel<false, true> : preprocess_kernel<false, false>));
    for (int v = v0; v < views; ++v) {
        const ViewCams<1> c = view_cams<1>(viewmatrix, projmatrix, campos, cs, v, 1);
        const size_t og = pv * v, oa = pa * v;
        hipLaunchKernelGGL(kernel, grid, block, lds, s, *prm, at(means3D, 3, og), shs, at(colors_precomp, 3, oa), opacities + oa,
                           at(scales, 3, og), at(rotations, 4, og), at(cov3D_precomp, 6, og), c.vm[0], c.pm[0], c.cp[0],
                           geom_view(g, prm->P, v), bin.tile_count, bin.tile_count2, bin.vis_part, resv + resv_view * v,
                           radii + (size_t)prm->P * v, v * gyv);
    }
    return check_launch(s, prm->debug & 0xff);
}

extern "C" int d3ga_raster_recolor(const d3ga_raster_params *prm, const float *means3D, const float *shs,
                                   const float *colors_precomp, const float *campos, const void *geom_src,
                                   void *geom_dst, d3ga_stream_t stream) {
    D3GA_TRY(validate(prm));
    if (n_views_of(prm) > 1 || is_windowed(prm)) return D3GA_E_CONFIG;
    if (prm->P == 0) return D3GA_OK;
    if (!geom_src || !geom_dst || geom_src == geom_dst) return D3GA_E_NULL;
    if ((shs != nullptr) == (colors_precomp != nullptr)) return D3GA_E_CONFIG;
    if (shs && (!means3D || !campos)) return D3GA_E_NULL;
    if (shs && (prm->sh_degree + 1) * (prm->sh_degree + 1) > prm->M) return D3GA_E_CONFIG;
    hipStream_t s = (hipStream_t)stream;
    const GeomBuf src = carve_geom(const_cast<void *>(geom_src), prm->P), dst = carve_geom(geom_dst, prm->P);
    hipLaunchKernelGGL(leaves_dcol(prm, shs) ? recolor_kernel<true> : recolor_kernel<false>, dim3((prm->P + kBlock - 1) / kBlock),
                       dim3(kBlock), lds_bytes(staged(prm, shs), kShHalfLdsBytes), s, *prm, means3D, shs, colors_precomp, campos, src, dst);
    return check_launch(s, prm->debug & 0xff);
}

// R6 with the deform backward as its tail (preprocess_bwd_kernel<false, true>): one view on the full raster, a precomputed
// covariance -- the deform's output.  dL_dmeans3D / dL_dcov3D may be null (not written).  The vertex gather and the skinning / pose
// tails are d3ga_cage_deform_bwd_tail's, on the records this leaves.
extern "C" int d3ga_raster_preprocess_bwd_deform(const d3ga_raster_params *prm, const float *means3D, const float *shs,
                                                 const float *scales, const float *rotations, const float *cov3D_precomp,
                                                 const float *viewmatrix, const float *projmatrix, const float *campos,
                                                 const void *geom, const float *acc, float *dL_dmeans3D, float *dL_dmeans2D,
                                                 float *dL_dopacity, float *dL_dsh, float *dL_dcolors, float *dL_dcov3D,
                                                 float *dL_dscales, float *dL_drots, const d3ga_cage_deform_in *din,
                                                 const d3ga_cage_deform_grads *dgr, const d3ga_cage_deform_route *route,
                                                 d3ga_stream_t stream) {
    D3GA_TRY(validate(prm));
    D3GA_TRY(deform_tail_check(din, dgr, route));
    if (n_views_of(prm) > 1 || is_windowed(prm) || scales || rotations || dL_dscales || dL_drots || din->P != prm->P) return D3GA_E_CONFIG;
    if ((dL_dmeans3D != nullptr) != (dL_dcov3D != nullptr)) return D3GA_E_CONFIG;      // both arrays or neither
    if (prm->P == 0) return D3GA_OK;
    if (!means3D || !viewmatrix || !projmatrix || !campos || !geom || !acc || !cov3D_precomp) return D3GA_E_NULL;
    if (dL_dsh && !shs) return D3GA_E_NULL;
    if (shs && !dL_dsh && !dL_dcolors) return D3GA_E_NULL;
    hipStream_t s = (hipStream_t)stream;
    const GeomBuf g = carve_geom(const_cast<void *>(geom), prm->P);
    const bool merge = route && route->kind == D3GA_DEFORM_ROUTE_MERGE;
    // the SH slabs, and in their place the merge planes
    const size_t lds = lds_bytes(staged(prm, shs), kShLdsBytes, merge ? sizeof(float) * 3 * kMergeItems : 0);
    const ViewCams<1> c = view_cams<1>(viewmatrix, projmatrix, campos, cam_stride(prm), 0, 1);
    auto launch = [&](auto dt) {
        using Tail = decltype(dt);
        dt = Tail{din->tetpoints, din->tetras, din->tetra_id, din->barys, din->canon_grad, din->scales, din->rots, din->delta_barys,
                  (int)din->flags, dgr->g_barys, dgr->g_scales, dgr->g_rots, (route && !merge) ? route->records : nullptr,
                  merge ? DeformMerge{route->item_pos, route->seg_ptr, route->seg_begin, route->records}
                        : DeformMerge{nullptr, nullptr, nullptr, nullptr}};
        hipLaunchKernelGGL((preprocess_bwd_kernel<false, true, Tail>), dim3((prm->P + kBlock - 1) / kBlock), dim3(kBlock), lds, s, *prm,
                           means3D, shs, (const float *)nullptr, (const float *)nullptr, c.vm[0], c.pm[0], c.cp[0], g, acc, dL_dmeans3D,
                           dL_dmeans2D, dL_dopacity, dL_dsh, dL_dcolors, dL_dcov3D, (float *)nullptr, (float *)nullptr, cov3D_precomp, 0, dt);
    };
    if (dL_dmeans3D) launch(DeformTailGeo{});
    else launch(DeformTail{});
    return check_launch(s, prm->debug);
}

extern "C" int d3ga_raster_preprocess_bwd(const d3ga_raster_params *prm, const float *means3D, const float *shs,
                                          const float *scales, const float *rotations, const float *cov3D_precomp,
                                          const float *viewmatrix, const float *projmatrix, const float *campos,
                                          const void *geom, const float *acc, float *dL_dmeans3D, float *dL_dmeans2D,
                                          float *dL_dopacity, float *dL_dsh, float *dL_dcolors, float *dL_dcov3D,
                                          float *dL_dscales, float *dL_drots, d3ga_stream_t stream) {
    D3GA_TRY(validate(prm));
    if (prm->P == 0) return D3GA_OK;
    if (!means3D || !viewmatrix || !projmatrix || !campos || !geom || !acc || !dL_dmeans3D) return D3GA_E_NULL;
    if (dL_dsh && !shs) return D3GA_E_NULL;
    if (shs && !dL_dsh && !dL_dcolors) return D3GA_E_NULL;        // SH path: full block or factored (P,3) output
    if ((dL_dscales != nullptr) != (dL_drots != nullptr)) return D3GA_E_CONFIG;
    if (dL_dscales && (!scales || !rotations)) return D3GA_E_NULL;
    // the covariance the forward worked with: built from (scales, rotations) -> the geometry record holds it; precomputed -> the
    // forward kept NO copy (ABI 101), the caller's tensor is read again: a NULL here would mean uninitialised records
    if (!cov3D_precomp && !(scales && rotations)) return D3GA_E_NULL;
    hipStream_t s = (hipStream_t)stream;
    const int views = n_views_of(prm);
    const bool pva = views > 1 && prm->per_view_appearance;      // per-view opacity / colour gradients: precomputed colours only (d3ga.h)
    if (pva && shs) return D3GA_E_CONFIG;
    const GeomBuf g = carve_geom(const_cast<void *>(geom), (int64_t)prm->P * views);
    const size_t lds = lds_bytes(staged(prm, shs), kShLdsBytes);
    const bool win = is_windowed(prm);
    const int cs = cam_stride(prm);
    const dim3 grid((prm->P + kBlock - 1) / kBlock), block(kBlock);
    const size_t pv = prm->per_view_geometry ? (size_t)prm->P : 0;      // a batch of frames: every view has its own geometry and geometry gradients
    // one view of the batch on ITS records (preprocess_bwd_kernel)
    auto launch_view = [&](int v, float *dsh, float *dcol, int accum) {
        const ViewCams<1> c = view_cams<1>(viewmatrix, projmatrix, campos, cs, v, 1);
        const size_t o = (size_t)prm->P * v, og = pv * v;
        hipLaunchKernelGGL(win ? preprocess_bwd_kernel<true> : preprocess_bwd_kernel<false>, grid, block, lds, s, *prm, at(means3D, 3, og),
                           shs, at(scales, 3, og), at(rotations, 4, og), c.vm[0], c.pm[0], c.cp[0], geom_view(g, prm->P, v),
                           acc + D3GA_ACC_STRIDE * o, dL_dmeans3D + 3 * og, at(dL_dmeans2D, 3, o), dL_dopacity, dsh, dcol,
                           at(dL_dcov3D, 6, og), at(dL_dscales, 3, og), at(dL_drots, 4, og), at(cov3D_precomp, 6, og), accum);
    };
    if (views == 1) {
        launch_view(0, dL_dsh, dL_dcolors, 0);
        return check_launch(s, prm->debug);
    }
    // k views: one pass over the Gaussians walks the views (preprocess_bwd_views_kernel), up to eight per launch -- when the SH
    // gradient is wanted as the (P,M,3) block (not as the factors of the camera-sharded exchange) and, for SH colours, the forward
    // left its direction Jacobian
    if (shs ? (dL_dsh != nullptr && leaves_dcol(prm, shs)) : true) {
        for (int v0 = 0; v0 < views; v0 += kMaxGroup) {
            const int kv = views - v0 < kMaxGroup ? views - v0 : kMaxGroup;
            const size_t o = (size_t)prm->P * v0, og = pv * v0, oa = pva ? o : 0;      // oa: the group's first per-view opacity / colour gradient
            hipLaunchKernelGGL(win ? preprocess_bwd_views_kernel<true> : preprocess_bwd_views_kernel<false>, grid, block, lds, s, *prm, kv,
                               at(means3D, 3, og), shs != nullptr, at(scales, 3, og), at(rotations, 4, og), at(cov3D_precomp, 6, og),
                               view_cams<kMaxGroup>(viewmatrix, projmatrix, campos, cs, v0, kv), geom_view(g, prm->P, v0),
                               acc + D3GA_ACC_STRIDE * o, dL_dmeans3D + 3 * og, at(dL_dmeans2D, 3, o), at(dL_dopacity, 1, oa), dL_dsh,
                               at(dL_dcolors, 3, oa), at(dL_dcov3D, 6, og), at(dL_dscales, 3, og), at(dL_drots, 4, og), v0 > 0, pv, pva);
        }
        return check_launch(s, prm->debug);
    }
    // otherwise: one launch per view on ITS records; view 0 writes the gradients of the view-independent
    if (pva) return D3GA_E_CONFIG;                                 // (SH colours only come here: per-view appearance is refused above)
    if (shs && !dL_dcolors) return D3GA_E_NULL;
    if (prm->factor_rows != 0 && prm->factor_rows < prm->P) return D3GA_E_SIZE;
    const size_t fr = prm->factor_rows > 0 ? (size_t)prm->factor_rows : (size_t)prm->P;      // rows between the views' SH factors
    for (int v = 0; v < views; ++v) launch_view(v, nullptr, shs ? dL_dcolors + 3 * fr * v : dL_dcolors, v > 0 ? (pv ? 1 : 3) : 0);
    D3GA_TRY(check_launch(s, prm->debug));
    if (shs && dL_dsh) {
        hipLaunchKernelGGL(sh_grad_from_views_kernel, grid, block, lds_bytes(sh_staged(prm->M), kShLdsBytes), s, prm->P, prm->M,
                           prm->sh_degree, views, means3D, (int64_t)(3 * pv), dL_dcolors, (int64_t)(3 * fr), campos, (int64_t)cs, 1.0f, dL_dsh);
        return check_launch(s, prm->debug);
    }
    return D3GA_OK;
}

extern "C" int d3ga_sh_grad_from_views(int32_t P, int32_t M, int32_t sh_degree, int32_t n_views, const float *means3D,
                                       const float *g_views, int64_t g_stride, const float *campos_views,
                                       int64_t campos_stride, float scale, float *dL_dsh, d3ga_stream_t stream) {
    if (P < 0 || M < 1 || M > 16 || n_views < 0) return D3GA_E_SIZE;
    if (sh_degree < 0 || sh_degree > 3 || (sh_degree + 1) * (sh_degree + 1) > M) return D3GA_E_CONFIG;
    if (P == 0) return D3GA_OK;
    if (!means3D || !dL_dsh || (n_views > 0 && (!g_views || !campos_views))) return D3GA_E_NULL;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sh_grad_from_views_kernel, dim3((P + kBlock - 1) / kBlock), dim3(kBlock), lds_bytes(sh_staged(M), kShLdsBytes), s, P, M, sh_degree,
                       n_views, means3D, (int64_t)0, g_views, g_stride, campos_views, campos_stride, scale, dL_dsh);
    return check_launch(s, 0);
}

extern "C" int d3ga_raster_mark_visible(int32_t P, const float *means3D, const float *viewmatrix, uint8_t *visible,
                                        d3ga_stream_t stream) {
    if (P < 0) return D3GA_E_SIZE;
    if (P == 0) return D3GA_OK;
    if (!means3D || !viewmatrix || !visible) return D3GA_E_NULL;
    hipLaunchKernelGGL(mark_visible_kernel, dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0, (hipStream_t)stream, P,
                       means3D, viewmatrix, visible);
    return check_launch((hipStream_t)stream, 0);
}
