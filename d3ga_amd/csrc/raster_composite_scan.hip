// raster_composite_scan.hip -- compositing backward: composite_bwd_tile_kernel.
//
// Entry per lane, workgroup per tile.  The forward (raster_composite.hip) leaves, per 4x4 pixel block, the culled list of
// the entries that can touch it (ImgBuf::blk_list: {1-based position in the tile list, Gaussian index}).  Here
//   * one 256-thread workgroup owns a 16x16 tile; each of its four wavefronts takes four blocks (the tile's 16 blocks sorted
//     by list length, ranks 4g .. 4g+3 per wavefront: kDefaultTileAssign) and each 16-lane DPP row walks ITS block's list
//     back to front, 16 consecutive entries in its 16 lanes ("group"), stepping through the block's 16 pixels;
//   * what couples the entries at one pixel is the transmittance T_i = T_final / prod_{j >= i}(1 - alpha_j) and the colour
//     blended behind entry i, S_i = sum_{j > i} (c_j . dL/dpixel) alpha_j T_j -- two PREFIX SCANS over the row (row_shr:1,2,4,8,
//     four pixels interleaved by hand), the pixel's running (T, S) carried from group to group in a 32-byte LDS record;
//     dL/dalpha_i = T_i (c_i . g) - (S_i + T_final (bg . g)) / (1 - alpha_i): algebraically upstream's accum_rec recurrence;
//   * every lane accumulates the nine moments of ITS entry over the 16 pixels in registers (no cross-lane reduction); the
//     geometric ones centred as they are summed (the pixels' own dx, the line's own dy);
//   * the records of a tile's 16 blocks meet in a position-keyed MERGE CACHE in LDS (S slots of 12 dwords, slot =
//     (position - 1) mod S; the tag word is the slot's lock, taken with ONE returning integer LDS atomic per attempt --
//     float LDS atomics are 46x slower on this part) before one 64-byte accumulator line per (tile, Gaussian) leaves the CU
//     as float atomics; displaced records (live window wider than S) leave early;
//   * a wavefront that is done leaves; the last one of the tile to arrive (an LDS counter) publishes the cache;
//   * alpha is evaluated by the same splat_eval_q() as the forward and the validity test is the forward's (power <= 0,
//     alpha >= 1/255, list position <= the pixel's n_contrib): the set of (pixel, entry) pairs is exactly the forward's.
// Optionally the L1 image-loss gradient is formed per pixel here (d3ga_raster_backward_l1) and a second image's gradient
// is folded in (DUAL: render_pair).  Numbers, history and the negative results: DESIGN.md sec. 4.
#include "composite_common.h"

// D3GA_SCAN_ABL: timing ablations of the kernel below (ablation builds only -- tools/_build/, results are WRONG, the Python
// layer refuses them unless D3GA_ALLOW_ABLATION=1; tools/gpu_ablate.sh):
//   1 nothing leaves the CU and no inserts | 8 every insert but no pixel steps | 12 rows not paced | 13 inserts but nothing leaves the CU
#ifndef D3GA_SCAN_ABL
#define D3GA_SCAN_ABL 0
#endif
// tile kernel only: 13 cache inserts but nothing leaves the CU; D3GA_TILE_WAVES: wavefronts per SIMD the register budget targets
#ifndef D3GA_TILE_WAVES
#define D3GA_TILE_WAVES 4
#endif
#ifndef D3GA_TILE_PRIO
#define D3GA_TILE_PRIO 0
#endif

namespace d3ga {

// Inclusive scans over the 16 lanes of a DPP row (row_shr:1, 2, 4, 8), FOUR independent values at once: the four chains
// are interleaved by hand so that the two wait states a DPP read needs after the VALU write of its source are filled with
// useful instructions instead of s_nop (the compiler serialises the chains and pads every step).
//   mul: v_mul_f32_dpp d, d(shifted), d with bound_ctrl:0 -- a lane without a source lane is disabled and keeps d.
//   add: bound_ctrl:1 -- a lane without a source lane adds 0.
#define D3GA_SCAN4(OP, BC, N) \
    OP " %0, %0, %0 row_shr:" #N " row_mask:0xf bank_mask:0xf" BC "\n" \
    OP " %1, %1, %1 row_shr:" #N " row_mask:0xf bank_mask:0xf" BC "\n" \
    OP " %2, %2, %2 row_shr:" #N " row_mask:0xf bank_mask:0xf" BC "\n" \
    OP " %3, %3, %3 row_shr:" #N " row_mask:0xf bank_mask:0xf" BC "\n"
// R rows per block (R = 2, 4: a block's list runs over 32 / 64 lanes): the row scans are continued across the rows with
// row_bcast:15 (lane 15 of a row -> every lane of the next row; row_mask 0xa: rows 1 and 3 take it) and, for R = 4,
// row_bcast:31 (lane 31 -> rows 2 and 3) -- the wave-wide scan idiom of this ISA family, two more steps per chain.
#define D3GA_SCANX(OP, CTRL, MASK) \
    OP " %0, %0, %0 " CTRL " row_mask:" MASK " bank_mask:0xf\n" \
    OP " %1, %1, %1 " CTRL " row_mask:" MASK " bank_mask:0xf\n" \
    OP " %2, %2, %2 " CTRL " row_mask:" MASK " bank_mask:0xf\n" \
    OP " %3, %3, %3 " CTRL " row_mask:" MASK " bank_mask:0xf\n"
template <int R = 1>
__device__ __forceinline__ void row_scan_mul4(float &a, float &b, float &c, float &d) {
    asm("s_nop 1\n" D3GA_SCAN4("v_mul_f32_dpp", "", 1) D3GA_SCAN4("v_mul_f32_dpp", "", 2) D3GA_SCAN4("v_mul_f32_dpp", "", 4)
        D3GA_SCAN4("v_mul_f32_dpp", "", 8)
        : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
    if constexpr (R >= 2) asm("s_nop 1\n" D3GA_SCANX("v_mul_f32_dpp", "row_bcast:15", "0xa") : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
    if constexpr (R >= 4) asm("s_nop 1\n" D3GA_SCANX("v_mul_f32_dpp", "row_bcast:31", "0xc") : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
}
template <int R = 1>
__device__ __forceinline__ void row_scan_add4(float &a, float &b, float &c, float &d) {
    asm("s_nop 1\n" D3GA_SCAN4("v_add_f32_dpp", " bound_ctrl:1", 1) D3GA_SCAN4("v_add_f32_dpp", " bound_ctrl:1", 2)
        D3GA_SCAN4("v_add_f32_dpp", " bound_ctrl:1", 4) D3GA_SCAN4("v_add_f32_dpp", " bound_ctrl:1", 8)
        : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
    if constexpr (R >= 2) asm("s_nop 1\n" D3GA_SCANX("v_add_f32_dpp", "row_bcast:15", "0xa") : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
    if constexpr (R >= 4) asm("s_nop 1\n" D3GA_SCANX("v_add_f32_dpp", "row_bcast:31", "0xc") : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
}

typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));
// (vector types: each load's registers stay one tuple that the prefetch fills in place -- as scalars the compiler may give
// them scattered registers and copy them over right behind the load, waiting for it)
struct ScanEntry {          // one list entry as the lane that owns it holds it
    uint32_t pos, gid;      // 1-based position in the tile list (0: no entry), Gaussian index
    f2 xy;
    f4 co;                  // conic a, b, c | opacity
    f4 rgb;                 // colour | 1/depth (unused here)
    float c2r, c2g, c2b;    // DUAL: the second image's colour
};

// Loads the entry pg into e.  A lane without an entry (pg.x = 0) loads nothing and keeps what e held (zeros, or an entry of
// an earlier group: finite values) -- the validity test's list-position term rejects it at every pixel (composite below), so no
// zeroing and no copies are needed here.
template <bool DUAL>
__device__ __forceinline__ void scan_gather(ScanEntry &e, uint2 pg, const float2 *__restrict__ xy, const float4 *__restrict__ conic_o,
                                            const float4 *__restrict__ rgb_invd, const float *__restrict__ colors2 /* DUAL: already moved back by 3 x view x P (the lists hold (view, Gaussian) indices, colors2 is per Gaussian) */) {
    e.pos = pg.x; e.gid = pg.y;
    if (pg.x != 0u) {
        e.xy = *reinterpret_cast<const f2 *>(xy + 2 * (size_t)pg.y);      // xy: the xyh records viewed as float2 (stride 2)
        e.co = *reinterpret_cast<const f4 *>(conic_o + pg.y);
        e.rgb = *reinterpret_cast<const f4 *>(rgb_invd + pg.y);
        if constexpr (DUAL) {
            e.c2r = colors2[3 * (size_t)pg.y]; e.c2g = colors2[3 * (size_t)pg.y + 1]; e.c2b = colors2[3 * (size_t)pg.y + 2];
        }
    }
}

#ifdef D3GA_DIAG
__device__ unsigned long long g_diag_scan[16];    // diagnostic build only (tools/diag_scan.py): loop statistics of the kernel below
__device__ unsigned long long g_diag_waves[32768 * 4];   // per active wave: s_memtime at start / end, groups, HW_ID | XCC_ID << 32
#endif
// forces the compiler's s_waitcnt for these registers HERE (an empty asm that reads them)
template <bool DUAL>
__device__ __forceinline__ void scan_consume(ScanEntry &e, uint2 &pg) {
    asm volatile("" : "+v"(e.xy), "+v"(e.co), "+v"(e.rgb), "+v"(pg.x), "+v"(pg.y));
    if constexpr (DUAL) asm volatile("" : "+v"(e.c2r), "+v"(e.c2g), "+v"(e.c2b));
}

typedef uint32_t u2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) uint32_t lds_u32;

// Everything the per-tile work of one wavefront reads (the kernels' pointer arguments, by value).
struct BwdArgs {
    int W, H, gx, gyv, P;    // gyv: tile rows per view (view-batched launches: composite_common.h, Quad); P: Gaussians per view
    const float2 *xy; const float4 *conic_o; const float4 *rgb_invd; const float *bg; const float *final_T; const uint32_t *n_contrib;
    const float *dL_dpix; float *acc; const float *colors2; const float *bg2; const float *dL_dpix2; const uint2 *blk_list;
    const uint32_t *blk_count; L1Source l1; const float *dL_dinvd;
    const int4 *win;         // windowed camera slot: the window table ({ox, oy, w, h} per view), else null
};
struct BwdDiag { unsigned long long install = 0, hit = 0, evict = 0, valid = 0, entries = 0, rowgroups = 0, trips = 0, groups = 0; };

// One wavefront's share of one tile: its SEG = 4 / R blocks (`blk`: the block of THIS lane's segment, in the forward's numbering),
// walked back to front in groups of 16 R entries, every record merged into the tile's cache `s_cache` (see the file header).
// s_pix / s_dump: this wavefront's pixel records and staging area.
template <bool DUAL, int S, bool INVD, int R, bool WIN>
__device__ __forceinline__ void bwd_tile_wave(const BwdArgs &A, const int tile, const uint32_t begin, const uint32_t end, const int blk,
                                              uint32_t *const s_cache, float *const s_pix, float *const s_dump, const int lane,
                                              BwdDiag &dg) {
    constexpr int PIXF = DUAL ? 12 : 8;
    constexpr int ROWF = 16 * PIXF + 4;
    constexpr int kSlot = 12;                        // dwords per cache slot
    constexpr uint32_t kLocked = 0xffffffffu;
    constexpr int LW = 16 * R;
    const int row = lane / LW, l16 = lane & 15, lseg = lane & (LW - 1);      // row: which of the wavefront's blocks; lseg: lane within the block's group
    constexpr int kVals = INVD ? 10 : 9, kPerInst = 64 / kVals;           // publish: values per record, records per instruction
    const int fq = lane / kVals, fk = lane - kVals * fq;   // lane -> (record within a group of 7 (6), value)
    const int fk_off = fk < 2 ? fk : fk + 1;               // acc layout 0,1 | 3,4,5 | 6 | 7,8,9 | 10 (dL/d(1/depth), INVD)
    constexpr int kAccStride = D3GA_ACC_STRIDE;
    const int bx = 2 * ((blk >> 2) & 1) + (blk & 1), by = 2 * (blk >> 3) + ((blk >> 1) & 1);      // the forward numbers a tile's blocks 4 * quadrant + (block within the quadrant)
    const int tyb = tile / A.gx, view = tyb / A.gyv;                                          // tile row of the batch -> (view, row of the view)
    int4 wv = make_int4(0, 0, A.W, A.H);                         // WIN: {ox, oy, w, h} of the view (the grid starts at tile (ox / 16, oy / 16))
    if constexpr (WIN) wv = A.win[view];
    const int bx0 = (tile - tyb * A.gx) * kTile + 4 * bx + (WIN ? (wv.x & ~(kTile - 1)) : 0);
    const int by0 = (tyb - view * A.gyv) * kTile + 4 * by + (WIN ? (wv.y & ~(kTile - 1)) : 0);      // block origin in pixels (local to the view)
    const int px = bx0 + (l16 & 3), py = by0 + (l16 >> 2);
    const bool inside = WIN ? (px >= wv.x && px < wv.x + A.W && py >= wv.y && py < wv.y + A.H) : (px < A.W && py < A.H);
    const int ix = WIN ? px - wv.x : px, iy = WIN ? py - wv.y : py;      // the pixel in the W x H images
    const size_t hw = (size_t)A.H * A.W;
    const size_t pid1 = hw * view + (size_t)iy * A.W + ix;       // one-plane images (final_T, n_contrib, inverse depth) of the view
    const size_t pid = pid1 + 2 * hw * view;                     // three-plane images
    const float T_final = inside ? A.final_T[pid1] : 0.f;
    const uint32_t last = inside ? A.n_contrib[pid1] : 0u;
    float g0 = 0.f, g1 = 0.f, g2 = 0.f;
    if (inside && A.dL_dpix) { g0 = A.dL_dpix[pid]; g1 = A.dL_dpix[hw + pid]; g2 = A.dL_dpix[2 * hw + pid]; }
    if (inside && A.l1.image) {
        // fused L1 image loss (d3ga_raster_backward_l1): dL/dpixel += dL/dloss / n * sign(image - target), formed here
        // instead of being written to and read back from a (3,A.H,A.W) gradient image
        const float *tgt = A.l1.target_cell ? *A.l1.target_cell : A.l1.target;
        const float sc = A.l1.g_loss[0] * A.l1.inv_n;
        auto sgn = [](float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); };
        g0 += sc * sgn(A.l1.image[pid] - tgt[pid]);
        g1 += sc * sgn(A.l1.image[hw + pid] - tgt[hw + pid]);
        g2 += sc * sgn(A.l1.image[2 * hw + pid] - tgt[2 * hw + pid]);
    }
    float bg_dot = A.bg[0] * g0 + A.bg[1] * g1 + A.bg[2] * g2;
    float h0 = 0.f, h1 = 0.f, h2 = 0.f;
    if constexpr (DUAL) {
        if (inside) { h0 = A.dL_dpix2[pid]; h1 = A.dL_dpix2[hw + pid]; h2 = A.dL_dpix2[2 * hw + pid]; }
        bg_dot += A.bg2[0] * h0 + A.bg2[1] * h1 + A.bg2[2] * h2;
    }
    const uint32_t maxlast = wave_max_u32(last);
    if (maxlast == 0) return;

    float *const pixrow = s_pix + row * ROWF;
    float *const wr_base = lseg == LW - 1 ? pixrow : s_dump + 2 * lane;
    {
        float *rec = pixrow + l16 * PIXF;
        *reinterpret_cast<float4 *>(rec) = make_float4(T_final, T_final * bg_dot, g0, g1);      // (T, S + T_final (bg . g)) carried
        float gd = 0.f;
        if constexpr (INVD) gd = inside ? A.dL_dinvd[pid1] : 0.f;
        *reinterpret_cast<float4 *>(rec + 4) = make_float4(g2, 0.f, __uint_as_float(last), gd);
        if constexpr (DUAL) *reinterpret_cast<float4 *>(rec + 8) = make_float4(h0, h1, h2, 0.f);
    }
    const uint32_t blk_cap = end - begin;
    // (the forward writes A.blk_count only for quadrants that start inside the image)
    const int qx0 = bx0 - 4 * (bx & 1), qy0 = by0 - 4 * (by & 1);
    const bool quad_in = WIN ? (qx0 < wv.x + A.W && qy0 < wv.y + A.H && qx0 + 8 > wv.x && qy0 + 8 > wv.y) : (qx0 < A.W && qy0 < A.H);
    const uint32_t cnt = quad_in ? A.blk_count[16 * (size_t)tile + blk] : 0u;
    const uint2 *const list = A.blk_list + 16 * (size_t)begin + (size_t)blk * blk_cap;
    const int ngroups = (int)((wave_max_u32(cnt) + (uint32_t)(LW - 1)) / (uint32_t)LW);
    const float ddelx_dx = 0.5f * (WIN ? wv.z : A.W), ddely_dy = 0.5f * (WIN ? wv.w : A.H);      // d(pixel)/d(ndc) of the full raster
    const float bxr = (float)bx0, byr = (float)by0;
    const int per = D3GA_SCAN_ABL == 12 ? LW : (ngroups > 0 ? ((int)cnt + ngroups - 1) / ngroups : 0);      // rows paced to finish together (see above)
    auto list_entry = [&](int g) -> uint2 {
        const int idx = (int)cnt - 1 - per * g - lseg;
        uint2 v = list[max(idx, 0)];
        v.x = (idx >= 0 && lseg < per) ? v.x : 0u;
        return v;
    };
    const float *const colors2v = DUAL ? A.colors2 - 3 * (size_t)view * (size_t)A.P : nullptr;
    ScanEntry e0, e1;
    e0.xy = f2{0.f, 0.f};
    e0.co = f4{0.f, 0.f, 0.f, 0.f};
    e0.rgb = f4{0.f, 0.f, 0.f, 0.f};
    e0.c2r = e0.c2g = e0.c2b = 0.f;
    scan_gather<DUAL>(e0, list_entry(0), A.xy, A.conic_o, A.rgb_invd, colors2v);
    e1 = e0;
    uint2 pg1 = list_entry(1);
    __builtin_amdgcn_wave_barrier();

    // One group: entry e (loaded one group ahead into nxt, list entries two groups ahead).  The loop below runs two groups per
    // trip with the roles of e0 and e1 swapped, so the prefetch lands in place: no register copies between groups and no
    // wait on the loads before the group's work (a rotation e = nxt made the compiler copy the loaded registers right
    // behind the loads).
    auto group = [&](ScanEntry &e, ScanEntry &nxt, const int g) {
        scan_gather<DUAL>(nxt, pg1, A.xy, A.conic_o, A.rgb_invd, colors2v);
        uint2 pg2 = list_entry(g + 2);
        const bool act = e.pos != 0u;
        const float exr = e.xy.x - bxr, eyr = e.xy.y - byr;
        const ConicQ cq = conic_q(e.co.x, e.co.y, e.co.z);
        // Geometric moments with the weight gop = o G dL/dalpha (dL/do = sum G dL/dalpha: divided by o once per entry), CENTRED as they
        // are summed: a block line adds  A = sum gop,  Bx = sum dx gop,  Cx = sum dx^2 gop  with the pixels' own dx = exr - k (and their
        // squares, formed once per group), and the line's own dy = eyr - ky weighs them into sum dy A, sum dy Bx, sum dy^2 A.  Every
        // sum is then a sum of its own terms and its rounding error is a few ulp of sum |terms|.  (Until this change the sums were
        // taken about the block's origin with k, ky as immediates and centred at the end of the group -- exr^2 SA - 2 exr SB + SC --,
        // six instructions per line fewer, but with an error of (offset of the centre from the block origin)^2 x sum gop whatever
        // the moment's own size: for a splat half a pixel thin, dL/dconic.c came out 6e-4 of itself off, LOG "Compositing: every
        // launch path under test".)
        float SA = 0.f, M0 = 0.f, M1 = 0.f, M2 = 0.f, M3 = 0.f, M4 = 0.f, M6 = 0.f, M7 = 0.f, M8 = 0.f, M9 = 0.f;
#if D3GA_TILE_PRIO
        {   // (the priority is an immediate)
            const int left = ngroups - g;
            if (left > 8) __builtin_amdgcn_s_setprio(3);
            else if (left > 4) __builtin_amdgcn_s_setprio(2);
            else if (left > 2) __builtin_amdgcn_s_setprio(1);
            else __builtin_amdgcn_s_setprio(0);
        }
#endif
        float dx[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) dx[k] = exr - (float)k;
        const float dxx[4] = {dx[0] * dx[0], dx[1] * dx[1], dx[2] * dx[2], dx[3] * dx[3]};
        // The four block lines, unrolled (record offsets and k, ky are immediates; no loop bookkeeping).  Per pixel step:
        //   * one select: an invalid pair gets o G = 0, so alpha = 0 (r = 1) and the pair's weight Gr = o G r is 0 too --
        //     its gradient terms vanish through the products that are already there;
        //   * the record carries S + T_final (bg . g) (the prologue seeds it), and with the INCLUSIVE colour-behind sum
        //     S' = S_i + u_i + T_final (bg . g), u_i = alpha_i T_i (c_i . g), dL/dalpha_i = T_i (c . g) - (S_i + T_final (bg . g)) r_i
        //     is (T_i (c . g) - S') r_i exactly (T_i (c . g) - u_i = T_i (c . g) / r_i): one fma, and r_i folds into Gr;
        //   * the geometric moments carry the opacity (Gr = o G r): the per-entry factor o is gone, dL/do = SA / o.
#pragma unroll
        for (int ky = 0; ky < (D3GA_SCAN_ABL == 8 ? 0 : 4); ++ky) {
            const float *const pixq = pixrow + ky * 4 * PIXF;
            float4 pa[4], pb[4], pc[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                pa[k] = *reinterpret_cast<const float4 *>(pixq + k * PIXF);
                pb[k] = *reinterpret_cast<const float4 *>(pixq + k * PIXF + 4);
                if constexpr (DUAL) pc[k] = *reinterpret_cast<const float4 *>(pixq + k * PIXF + 8);
                // the whole record is loaded HERE: left alone the compiler sinks the load of the colour gradient into a
                // divergent region -- an LDS round trip in the middle of every block line
                asm volatile("" : "+v"(pb[k].x), "+v"(pb[k].z));
                if constexpr (INVD) asm volatile("" : "+v"(pb[k].w));
            }
            const float dy = eyr - (float)ky;
            const float tb = cq.b * dy, tc = (cq.c * dy) * dy;
            float al[4], Gr[4], cgv[4], r4[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                // alpha as the forward forms it (splat_eval_q: p, G = exp2(p), alpha = min(kAlphaMax, o G)) and the forward's
                // test (p <= 0, alpha >= 1/255 -- for alpha = min(kAlphaMax, o G) the same as o G >= 1/255 --, list
                // position <= the pixel's n_contrib); a lane without an entry (pos = 0) is never valid
                float alpha, G;
                bool ok;
                splat_eval_q(dx[k], tb, tc, cq.a, e.co.w, alpha, G, ok);
                const float p = fmaf(dx[k], fmaf(cq.a, dx[k], tb), tc);      // (splat_eval_q's log2 G: the same instructions)
                const float oG = e.co.w * G;
                const bool valid = (p <= 0.0f) & (oG >= kAlphaMin) & (e.pos - 1u < __float_as_uint(pb[k].z));   // pos <= n_contrib, and never for pos = 0
#ifdef D3GA_DIAG_COUNTERS
                dg.valid += valid ? 1 : 0;          // lane efficiency: valid (entry, pixel) pairs / issued lane slots
#endif
                const float oGv = valid ? oG : 0.f;
                al[k] = fminf(kAlphaMax, oGv);                                     // == alpha where valid, else 0
                const float r = __builtin_amdgcn_rcpf(1.0f - al[k]);
                Gr[k] = oGv * r;
                cgv[k] = e.rgb.x * pa[k].z + e.rgb.y * pa[k].w + e.rgb.z * pb[k].x;
                if constexpr (DUAL) cgv[k] += e.c2r * pc[k].x + e.c2g * pc[k].y + e.c2b * pc[k].z;
                if constexpr (INVD) cgv[k] = fmaf(e.rgb.w, pb[k].w, cgv[k]);
                r4[k] = r;
            }
            row_scan_mul4<R>(r4[0], r4[1], r4[2], r4[3]);
            float Ti[4], dch[4], s[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) { Ti[k] = pa[k].x * r4[k]; dch[k] = al[k] * Ti[k]; s[k] = cgv[k] * dch[k]; }
            row_scan_add4<R>(s[0], s[1], s[2], s[3]);
            float *const wq = wr_base + ky * 4 * PIXF;
            float gop[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float Sin = s[k] + pa[k].y;
                gop[k] = Gr[k] * fmaf(Ti[k], cgv[k], -Sin);
                M6 = fmaf(dch[k], pa[k].z, M6); M7 = fmaf(dch[k], pa[k].w, M7); M8 = fmaf(dch[k], pb[k].x, M8);
                if constexpr (INVD) M9 = fmaf(dch[k], pb[k].w, M9);
                *reinterpret_cast<float2 *>(wq + k * PIXF) = make_float2(Ti[k], Sin);
            }
            const float A = (gop[0] + gop[1]) + (gop[2] + gop[3]);
            const float Bx = fmaf(dx[3], gop[3], fmaf(dx[2], gop[2], fmaf(dx[1], gop[1], dx[0] * gop[0])));
            const float Cx = fmaf(dxx[3], gop[3], fmaf(dxx[2], gop[2], fmaf(dxx[1], gop[1], dxx[0] * gop[0])));
            const float dyy = dy * dy;
            // (the lines are unrolled: the first one sets the sums)
            if (ky == 0) { SA = A; M0 = Bx; M2 = Cx; M1 = dy * A; M3 = dy * Bx; M4 = dyy * A; }
            else { SA += A; M0 += Bx; M2 += Cx; M1 = fmaf(dy, A, M1); M3 = fmaf(dy, Bx, M3); M4 = fmaf(dyy, A, M4); }
        }
        // dL/do = sum G dL/dalpha = SA / o (a lane whose opacity is below 1/255 has no valid pair: SA = 0)
        const float M5 = SA * __builtin_amdgcn_rcpf(fmaxf(e.co.w, kAlphaMin));
        const float v0 = -(e.co.x * M0 + e.co.y * M1) * ddelx_dx;
        const float v1 = -(e.co.z * M1 + e.co.y * M0) * ddely_dy;
        const float4 va = make_float4(v0, v1, -0.5f * M2, -0.5f * M3), vb = make_float4(-0.5f * M4, M5, M6, M7);
        scan_consume<DUAL>(nxt, pg2);
        __builtin_amdgcn_wave_barrier();
        // ---- merge into the tile's cache (see the header) ----
        // One LDS round trip per attempt: the exchange that takes the slot and the (speculative) loads of its record
        // are issued together -- LDS instructions of a wavefront execute in order, so the loads see the record as the
        // lock holder owns it; a loser discards them.  Stores + the releasing tag store likewise need no wait.
        const uint32_t saddr = (uint32_t)(uintptr_t)(lds_u32 *)(s_cache + ((e.pos - 1u) & (uint32_t)(S - 1)) * kSlot);
        // an entry that touched no pixel has nothing but (exact) zeros: it stays out of the cache
        const uint32_t anybits = (__float_as_uint(SA) | __float_as_uint(M0) | __float_as_uint(M2)) | (__float_as_uint(M1) | __float_as_uint(M3) | __float_as_uint(M4)) |
                                 (__float_as_uint(M6) | __float_as_uint(M7) | __float_as_uint(M8) | __float_as_uint(M9));
        bool pending = D3GA_SCAN_ABL == 1 ? (anybits == 0x12345u) : (D3GA_SCAN_ABL == 8 ? act : (anybits << 1) != 0u);
#ifdef D3GA_DIAG_TIMELINE
        dg.groups += 1;
#endif
#ifdef D3GA_DIAG_COUNTERS
        dg.entries += act ? 1 : 0;
        dg.rowgroups += (act && lseg == 0) ? 1 : 0;
#endif
        while (__builtin_amdgcn_ballot_w64(pending) != 0ull) {
#ifdef D3GA_DIAG_TIMELINE
            dg.trips += 1;
#endif
            // straight-line body (selects, no nested divergent regions and no state carried around the loop: the first
            // version's phi copies and mask bookkeeping cost ~150 VALU instructions per attempt, PMC-measured)
            uint32_t old;
            f4 ca, cb;
            u2 cc;
            asm("" : "=v"(old), "=v"(ca), "=v"(cb), "=v"(cc));       // defined, arbitrary: lanes that are not pending never look
            float c9 = 0.f;
            if constexpr (INVD) {
                asm("" : "=v"(c9));
                if (pending)
                    asm volatile("ds_wrxchg_rtn_b32 %0, %5, %6 offset:40\n"
                                 "ds_read_b128 %1, %5\n"
                                 "ds_read_b128 %2, %5 offset:16\n"
                                 "ds_read_b64 %3, %5 offset:32\n"
                                 "ds_read_b32 %4, %5 offset:44\n"
                                 "s_waitcnt lgkmcnt(0)"
                                 : "+v"(old), "+v"(ca), "+v"(cb), "+v"(cc), "+v"(c9)
                                 : "v"(saddr), "v"(kLocked)
                                 : "memory");
            } else
            if (pending)
                asm volatile("ds_wrxchg_rtn_b32 %0, %4, %5 offset:40\n"
                             "ds_read_b128 %1, %4\n"
                             "ds_read_b128 %2, %4 offset:16\n"
                             "ds_read_b64 %3, %4 offset:32\n"
                             "s_waitcnt lgkmcnt(0)"
                             : "+v"(old), "+v"(ca), "+v"(cb), "+v"(cc)
                             : "v"(saddr), "v"(kLocked)
                             : "memory");
            const bool won = pending && old != kLocked;
            const bool hit = won && old == e.pos;
            const bool evi = won && !hit && old != 0u;
#ifdef D3GA_DIAG_COUNTERS
            if (hit) dg.hit += 1; else if (evi) dg.evict += 1; else if (won) dg.install += 1;
#endif
            const f4 ta = {va.x + (hit ? ca.x : 0.f), va.y + (hit ? ca.y : 0.f), va.z + (hit ? ca.z : 0.f), va.w + (hit ? ca.w : 0.f)};
            const f4 tb4 = {vb.x + (hit ? cb.x : 0.f), vb.y + (hit ? cb.y : 0.f), vb.z + (hit ? cb.z : 0.f), vb.w + (hit ? cb.w : 0.f)};
            const u2 tc = {__float_as_uint(M8 + (hit ? __uint_as_float(cc.x) : 0.f)), e.gid};
            if constexpr (INVD) {
                const float t9 = M9 + (hit ? c9 : 0.f);
                if (won) asm volatile("ds_write_b32 %0, %1 offset:44" : : "v"(saddr), "v"(t9) : "memory");      // (before the tag store below releases the slot)
            }
            if (won)
                asm volatile("ds_write_b128 %0, %1\n"
                             "ds_write_b128 %0, %2 offset:16\n"
                             "ds_write_b64 %0, %3 offset:32\n"
                             "ds_write_b32 %0, %4 offset:40"
                             :
                             : "v"(saddr), "v"(ta), "v"(tb4), "v"(tc), "v"(e.pos)
                             : "memory");
            pending = pending && !won;
            const unsigned long long em = __builtin_amdgcn_ballot_w64(evi);
            if (em != 0ull) {
                // wave-uniform and rare (the window of live positions exceeded S): the displaced records leave through the
                // dump area, up to 20 at a time, nine (INVD: ten) consecutive lanes per record like every publish of this kernel
                const int rank = lanes_below(em), total = (int)__popcll(em);
                for (int c0 = 0; c0 < total; c0 += 20) {
                    if (evi && rank >= c0 && rank < c0 + 20) {
                        float *st = s_dump + (rank - c0) * 12;
                        st[0] = ca.x; st[1] = ca.y; st[2] = ca.z; st[3] = ca.w;
                        st[4] = cb.x; st[5] = cb.y; st[6] = cb.z; st[7] = cb.w;
                        st[8] = __uint_as_float(cc.x); st[9] = c9; st[10] = __uint_as_float(cc.y);      // value 9: dL/d(1/depth) (INVD), word 10: Gaussian id
                    }
                    const int n = min(total - c0, 20);
                    __builtin_amdgcn_wave_barrier();
                    for (int base = 0; base < n; base += kPerInst) {
                        const int ent = base + fq;
                        if (fq < kPerInst && ent < n) {
                            const float val = s_dump[ent * 12 + fk];
                            const uint32_t og = __float_as_uint(s_dump[ent * 12 + 10]);
                            if (D3GA_SCAN_ABL != 13 && val != 0.f) atomicAdd(A.acc + kAccStride * (size_t)og + fk_off, val);
                        }
                    }
                    __builtin_amdgcn_wave_barrier();
                }
            }
        }
        pg1 = pg2;
    };
    for (int g = 0; g < ngroups; g += 2) {
        group(e0, e1, g);
        if (g + 1 == ngroups) break;
        group(e1, e0, g + 1);
    }
}

// DUAL: a second image rendered with the same alphas (render_pair); S: slots of the tile's merge cache (see the file header).
// INVD: the inverse-depth image of branch dr_aa takes part as a fourth channel (its "colour" is the entry's 1 / depth): the
// incoming dL/dinvdepth joins c . g, and the entry's dL/d(1/depth) = sum alpha T dL/dinvdepth is a tenth accumulated value
// (the pad word of the cache slot, float 10 of the accumulator record).
// R: rows per block (D3GA_BWD_ROWS).  1: a wavefront's four rows walk four blocks, 16 entries per group and block, four
// wavefronts per tile.  2 / 4: 8 / 16 wavefronts per tile, a block's list runs over 2 / 4 rows (32 / 64 entries per group), a
// wavefront takes 2 / 1 blocks -- the same pixel steps in total, but the tile's longest list is walked in half / a quarter of
// the groups: the critical path of a heavy tile (18 groups of one wavefront at C3) shrinks with it.
template <bool DUAL, int S, bool INVD = false, int R = 1, bool PVB = false, bool WIN = false>      // PVB: bg is (k,3), one row per view (d3ga.h: per_view_background); WIN: windowed camera slot
__global__ __launch_bounds__(256 * R, (DUAL ? (D3GA_TILE_WAVES < 3 ? D3GA_TILE_WAVES : 3) : D3GA_TILE_WAVES)) void composite_bwd_tile_kernel(   // (DUAL: 12-float pixel records -- the LDS of three workgroups per CU)
   
    int W, int H, int gx, int gy, int gyv, const uint32_t *__restrict__ tile_start, uint64_t dcap, const float2 *__restrict__ xy,
    const float4 *__restrict__ conic_o, const float4 *__restrict__ rgb_invd, const float *__restrict__ bg,
    const float *__restrict__ final_T, const uint32_t *__restrict__ n_contrib, const float *__restrict__ dL_dpix,
    float *__restrict__ acc, const uint32_t *__restrict__ tile_order, const float *__restrict__ colors2,
    const float *__restrict__ bg2, const float *__restrict__ dL_dpix2, const uint2 *__restrict__ blk_list,
    const uint32_t *__restrict__ blk_count, int assign, L1Source l1, const float *__restrict__ dL_dinvd, int split_cap, const uint32_t *__restrict__ split_cnt, int P,
    const int4 *__restrict__ win) {
    static_assert((S & (S - 1)) == 0, "power of two");
    constexpr int NW = 4 * R;                        // wavefronts per tile (three, the third walking two sets of blocks: measured, slower -- DESIGN.md sec. 4)
    constexpr int SEG = 4 / R, LW = 16 * R;          // blocks per wavefront, lanes per block
    constexpr int PIXF = DUAL ? 12 : 8;
    constexpr int ROWF = 16 * PIXF + 4;
    constexpr int kSlot = 12;                        // dwords per cache slot
    const bool early_exit_off = (assign & 8) != 0;         // A/B: bit 3 of D3GA_TILE_ASSIGN keeps every wavefront until the tile is done
    assign &= 7;
    const int tiles = gx * gy;
    // split_h (D3GA_BWD_SPLIT, R = 1 only, needs the work order): each of the split_h heaviest tiles gets TWO workgroups -- the
    // even / odd ranks of its 16 blocks by length -- whose wavefronts take two blocks each over two rows (the R = 2 walk: 32
    // entries per group): the tile's longest list is walked in half the groups, at the price of a merge cache per half
    // The grid has room for split_cap of them; how many there are this frame is the order kernel's count (split_cnt; null: split_cap).
    int rank = (int)blockIdx.x, half = -1;
    if (R == 1 && split_cap > 0) {
        const int split_h = split_cnt ? min((int)*split_cnt, split_cap) : split_cap;
        if (rank < 2 * split_h) { half = rank & 1; rank >>= 1; } else rank -= split_h;
    }
    const int tile = tile_order ? (rank < tiles ? (int)tile_order[rank] : -1) : (rank < tiles ? rank : -1);
    if (tile < 0) return;                                  // uniform over the workgroup
    const uint32_t begin = (uint32_t)min((uint64_t)tile_start[tile], dcap);
    const uint32_t end = (uint32_t)min((uint64_t)tile_start[tile + 1], dcap);
    if (begin >= end) return;                              // uniform: empty tile

    __shared__ __attribute__((aligned(16))) float s_pix_all[NW][SEG * ROWF];
    __shared__ __attribute__((aligned(16))) float s_dump_all[NW][64 * 2 + 16 * PIXF];
    __shared__ __attribute__((aligned(16))) uint32_t s_cache[S * kSlot];
    // slot = (list position - 1) mod S: a list of n < S entries uses the first n slots only (init and publish stop there: a
    // third of the publish at C4, where lists average 340 entries)
    const int nslots = min(S, (int)(end - begin));
    for (int i = threadIdx.x; i < nslots; i += 64 * NW) s_cache[i * kSlot + 10] = 0u;   // tags: every slot empty
    __shared__ uint32_t s_arrived;                          // wavefronts of this tile that are done (the last one publishes the cache)
    if (threadIdx.x == 0) s_arrived = 0u;
    __shared__ uint8_t s_perm[16];                          // assign 2: the tile's 16 blocks by descending list length
    if (R > 1 || half >= 0) assign = 2;                     // (the quadrant / interleaved assignments exist for R = 1 only)
    if (assign == 2 && threadIdx.x < 16) {
        int4 wv = make_int4(0, 0, W, H);
        if constexpr (WIN) wv = win[(tile / gx) / gyv];
        const int b = threadIdx.x, tx0 = (tile % gx) * kTile + (WIN ? (wv.x & ~(kTile - 1)) : 0), ty0 = ((tile / gx) % gyv) * kTile + (WIN ? (wv.y & ~(kTile - 1)) : 0);
        auto count_of = [&](int j) -> uint32_t {            // (the forward writes the counts of quadrants that start inside the image)
            const int q = j >> 2, qx = tx0 + ((q & 1) << 3), qy = ty0 + ((q >> 1) << 3);
            const bool in = WIN ? (qx < wv.x + W && qy < wv.y + H && qx + 8 > wv.x && qy + 8 > wv.y) : (qx < W && qy < H);
            return in ? blk_count[16 * (size_t)tile + j] : 0u;
        };
        const uint32_t mine = count_of(b);
        int rank = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint32_t c = count_of(j);
            rank += (c > mine || (c == mine && j < b)) ? 1 : 0;
        }
        s_perm[rank] = (uint8_t)b;
    }
    __syncthreads();

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // block -> (wavefront, row).  assign 0: a wavefront takes the 2x2 blocks of one quadrant (the forward's grouping);
    // assign 1: it takes the blocks (wave & 1) + 2 i, (wave >> 1) + 2 j -- 8 pixels apart, so its rows rarely hold the same
    // Gaussian in the same group (copies that meet in ONE instruction serialise on the slot; copies in different wavefronts
    // simply hit the cache).  The forward numbers a tile's blocks 4 * quadrant + (block within the quadrant).
    // assign 2 (default): the four blocks of SIMILAR list length -- ranks 4 g .. 4 g + 3 of the tile's blocks sorted by length,
    // g = (wave + workgroup) mod 4.  A wavefront runs as many groups as its longest row needs, so rows of unequal length pad
    // (quadrants: 57.5 k wave-groups at C3, interleaved 59.3 k, against 49 k row-groups / 4); and rotating g with the workgroup
    // index gives every SIMD of a CU (wave w of a workgroup runs on SIMD w) one wavefront of each weight class.
    const int row = lane / LW;                             // which of the wavefront's blocks
    constexpr int kVals = INVD ? 10 : 9, kPerInst = 64 / kVals;           // publish: values per record, records per instruction
    const int fq = lane / kVals, fk = lane - kVals * fq;   // lane -> (record within a group of 7 (6), value)
    const int fk_off = fk < 2 ? fk : fk + 1;               // acc layout 0,1 | 3,4,5 | 6 | 7,8,9 | 10 (dL/d(1/depth), INVD)
    constexpr int kAccStride = D3GA_ACC_STRIDE;
    float *const s_pix = s_pix_all[wave];
    float *const s_dump = s_dump_all[wave];
    BwdDiag dg;
#ifdef D3GA_DIAG_TIMELINE
    const unsigned long long diag_t0 = __builtin_readcyclecounter(), diag_w0 = __builtin_amdgcn_s_memrealtime();
#endif

    {
        int blk;
        if (assign == 2) blk = s_perm[SEG * ((wave + (int)blockIdx.x) & (NW - 1)) + row];
        else {
            const int bx = assign ? 2 * (row & 1) + (wave & 1) : 2 * (wave & 1) + (row & 1);
            const int by = assign ? 2 * (row >> 1) + (wave >> 1) : 2 * (wave >> 1) + (row >> 1);
            blk = 4 * ((bx >> 1) + 2 * (by >> 1)) + ((bx & 1) + 2 * (by & 1));
        }
        const float *const bgv = PVB ? bg + 3 * ((tile / gx) / gyv) : bg;      // the tile's view: uniform over the workgroup
        const BwdArgs A = {W, H, gx, gyv, P, xy, conic_o, rgb_invd, bgv, final_T, n_contrib, dL_dpix, acc, colors2, bg2, dL_dpix2, blk_list, blk_count, l1, dL_dinvd, win};
        if (R == 1 && half >= 0) {
            blk = s_perm[2 * (2 * ((wave + (int)blockIdx.x) & 3) + (lane >> 5)) + half];
            bwd_tile_wave<DUAL, S, INVD, (R == 1 ? 2 : R), WIN>(A, tile, begin, end, blk, s_cache, s_pix, s_dump, lane, dg);
        } else
        bwd_tile_wave<DUAL, S, INVD, R, WIN>(A, tile, begin, end, blk, s_cache, s_pix, s_dump, lane, dg);
    }

#ifdef D3GA_DIAG_COUNTERS
    atomicAdd(&g_diag_scan[3], dg.install); atomicAdd(&g_diag_scan[4], dg.hit); atomicAdd(&g_diag_scan[5], dg.evict);
    atomicAdd(&g_diag_scan[8], dg.valid); atomicAdd(&g_diag_scan[9], dg.entries); atomicAdd(&g_diag_scan[10], dg.rowgroups);
#endif
#ifdef D3GA_DIAG_TIMELINE
    if (lane == 0 && dg.groups && blockIdx.x < 32768 / NW) {      // no atomics here: returning same-address atomics serialise at the memory side and would BE the timeline
        const unsigned long long diag_w1 = __builtin_amdgcn_s_memrealtime();
        const size_t slot = NW * (size_t)blockIdx.x + wave;
        g_diag_waves[4 * slot] = diag_w0 | ((__builtin_readcyclecounter() - diag_t0) << 40);
        g_diag_waves[4 * slot + 1] = diag_w1;
        g_diag_waves[4 * slot + 2] = dg.groups | (dg.trips << 16) | ((unsigned long long)(end - begin) << 32);
        g_diag_waves[4 * slot + 3] = (unsigned long long)__builtin_amdgcn_s_getreg(63492) | ((unsigned long long)(__builtin_amdgcn_s_getreg(6164) & 15) << 32);
    }
#endif
    // Publish.  A wavefront that is done LEAVES (its registers and wave slot go to the next workgroup: a tile's four
    // wavefronts take 5..18 groups, and with a closing barrier all four slots stayed occupied until the slowest was done --
    // the second dispatch round of the launch then started at half of the kernel's span, tools/diag_scan.py); the LAST one
    // to arrive (one returning integer LDS atomic per wavefront; LDS operations of a wavefront execute in order, so every
    // insert of a wavefront is complete when its arrival is counted) sends the whole cache to HBM, nine consecutive lanes
    // per record, seven records per instruction.
    if (D3GA_SCAN_ABL == 13 || D3GA_SCAN_ABL == 1) return;
    uint32_t arrived = 0u;
    // acq_rel at workgroup scope: this wavefront's cache stores are ordered BEFORE its arrival, and the publisher's reads of the
    // cache AFTER it has seen the others' arrivals -- by the memory model, not only by in-order LDS issue
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");       // every lane's cache stores (not only lane 0's) before the arrival
    if (lane == 0) arrived = __hip_atomic_fetch_add(&s_arrived, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    arrived = (uint32_t)__builtin_amdgcn_readfirstlane((int)arrived);
    if (arrived != (uint32_t)(NW - 1) && !early_exit_off) return;
    if (early_exit_off) { __syncthreads(); if (wave != 0) return; }
    for (int base = 0; base < nslots; base += kPerInst) {
        const int ent = base + min(fq, kPerInst - 1);
        const bool mine = fq < kPerInst && ent < nslots;
        const uint32_t *const sl = s_cache + min(ent, S - 1) * kSlot;
        const uint32_t tag = sl[10], gid = sl[9];
        const float val = __uint_as_float(sl[fk < 9 ? fk : 11]);
        if (mine && tag != 0u && val != 0.f) atomicAdd(acc + kAccStride * (size_t)gid + fk_off, val);
    }
}

#ifdef D3GA_DIAG
extern "C" __attribute__((visibility("default"))) int d3ga_diag_scan_read(unsigned long long *out16, int reset) {
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_diag_scan), sizeof(unsigned long long) * 16) != hipSuccess) return 1;
    if (reset) {
        unsigned long long z[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_diag_scan), z, sizeof(z)) != hipSuccess) return 1;
        void *w = nullptr;
        if (hipGetSymbolAddress(&w, HIP_SYMBOL(g_diag_waves)) != hipSuccess || hipMemset(w, 0, sizeof(unsigned long long) * 4 * 32768) != hipSuccess) return 1;
    }
    return 0;
}
extern "C" __attribute__((visibility("default"))) int d3ga_diag_scan_waves(unsigned long long *out, int n) {      // n <= 32768 records of 4 words
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_diag_waves), sizeof(unsigned long long) * 4 * (size_t)n) != hipSuccess;
}
#endif

int launch_composite_bwd_scan(const d3ga_raster_params *prm, int gx, int gy, const BinBuf &bin, const GeomBuf &g,
                              const ImgBuf &im, int64_t d_capacity, const float *bg, const float *dL_dpix, float *acc,
                              bool ordered, const float *colors2, const float *bg2, const float *dL_dpix2, const L1Source &l1,
                              hipStream_t s, const float *dL_dinvd) {
    // workgroup per tile, heaviest tiles first (tile_order of the bin stage); S = slots of the tile's merge cache
    const uint32_t *order = ordered ? (const uint32_t *)bin.tile_order : (const uint32_t *)nullptr;
    // split of the heaviest tiles (see the kernel): D3GA_BWD_SPLIT < 0 (default): the order kernel's count (a tenth of the non-empty
    // tiles, D3GA_CNT_HEAVY), read by every workgroup and capped by the grid's room for it; >= 0: that many (0: none)
    const int split_knob = composite_bwd_split();
    const int split_cap = !ordered ? 0 : (split_knob < 0 ? (gx * gy + 9) / 10 : min(split_knob, gx * gy));
    const uint32_t *split_cnt = (ordered && split_knob < 0) ? (const uint32_t *)(bin.counters + D3GA_CNT_HEAVY) : (const uint32_t *)nullptr;
    const dim3 tgrid(gx * gy + split_cap);
    const int S = composite_merge_slots();
    const bool pvb = n_views_of(prm) > 1 && prm->per_view_background;      // bg (k,3)
    const bool wnd = is_windowed(prm);
    const int4 *wtab = wnd ? win_table((void *)bin.counters, (int64_t)gx * gy, d_capacity) : nullptr;
#define D3GA_LAUNCH_TILE_R(DUALV, SV, INVDV, RV, PVBV, WINV)                                                                  \
    hipLaunchKernelGGL((composite_bwd_tile_kernel<DUALV, SV, INVDV, RV, PVBV, WINV>), tgrid, dim3(256 * RV),                    \
                       0, s, prm->W, prm->H, gx, gy, gy / n_views_of(prm), bin.tile_start, \
                       (uint64_t)d_capacity, reinterpret_cast<const float2 *>(g.xyh), g.conic_o, g.rgb_invd, bg, im.final_T, im.n_contrib, dL_dpix, acc, order,   \
                       colors2, bg2, dL_dpix2, (const uint2 *)im.blk_list, (const uint32_t *)im.blk_count, composite_tile_assign(), l1, dL_dinvd, split_cap, split_cnt, prm->P, wtab)
#define D3GA_LAUNCH_TILE(DUALV, SV, INVDV)                                                                                    \
    do {                                                                                                                      \
        if (wnd) { if (pvb) D3GA_LAUNCH_TILE_R(DUALV, SV, INVDV, 1, true, true); else D3GA_LAUNCH_TILE_R(DUALV, SV, INVDV, 1, false, true); } \
        else if (pvb) D3GA_LAUNCH_TILE_R(DUALV, SV, INVDV, 1, true, false);                                                   \
        else D3GA_LAUNCH_TILE_R(DUALV, SV, INVDV, 1, false, false);                                                           \
    } while (0)
    if (dL_dinvd) {                                          // inverse-depth gradient (branch dr_aa): single-image launches only
        if (colors2) return D3GA_E_CONFIG;
        if (S >= 512) D3GA_LAUNCH_TILE(false, 512, true); else D3GA_LAUNCH_TILE(false, 256, true);
    } else if (colors2) { if (S >= 512) D3GA_LAUNCH_TILE(true, 512, false); else D3GA_LAUNCH_TILE(true, 256, false); }
    else if (S >= 512) D3GA_LAUNCH_TILE(false, 512, false);
    else D3GA_LAUNCH_TILE(false, 256, false);
#undef D3GA_LAUNCH_TILE
#undef D3GA_LAUNCH_TILE_R
    return check_launch(s, prm->debug);
}

// test hook for the two row scans (d3ga_selftest_row_scan): lane l of every 16-lane row ends up with the inclusive sum /
// product of lanes 0..l of its row; the four chains of one call carry x, 2x, 3x, 4x (sums) and 1+x/8, 1+x/4, ... (products)
__global__ void row_scan_selftest_kernel(const float *__restrict__ in, float *__restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const float x = in[i];
    float a0 = x, a1 = 2.f * x, a2 = 3.f * x, a3 = 4.f * x;
    row_scan_add4(a0, a1, a2, a3);
    float m0 = 1.f + 0.125f * x, m1 = 1.f + 0.25f * x, m2 = 1.f + 0.375f * x, m3 = 1.f + 0.5f * x;
    row_scan_mul4(m0, m1, m2, m3);
    float *o = out + 8 * (size_t)i;
    o[0] = a0; o[1] = a1; o[2] = a2; o[3] = a3; o[4] = m0; o[5] = m1; o[6] = m2; o[7] = m3;
}

}  // namespace d3ga

extern "C" int d3ga_selftest_row_scan(int n, const float *in, float *out, d3ga_stream_t stream) {
    if (n <= 0 || (n % 256) != 0) return D3GA_E_SIZE;
    if (!in || !out) return D3GA_E_NULL;
    hipLaunchKernelGGL(d3ga::row_scan_selftest_kernel, dim3(n / 256), dim3(256), 0, (hipStream_t)stream, in, out, n);
    return d3ga::check_launch((hipStream_t)stream, 0);
}
