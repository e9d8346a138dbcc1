// png.hip -- PNG files of the recorder's written images: what torchvision.utils.save_image (test.py:182-195) and
// cv2.imwrite (train.py:371) do on a CPU thread after the uint8 image has crossed the bus -- filter, deflate, checksums, chunk
// framing -- as TWO launches on the image where compose_grid / to_uint8 left it, so that finished file bytes leave the device.
//
//   png_strip_kernel     a workgroup per strip of rows.  A wavefront per row chooses the filter (five sums of |int8|, butterfly
//                        shuffles) and writes the filtered bytes -- into LDS when the strip fits kPngLdsBytes, else into the
//                        scratch.  Then every thread owns a contiguous piece of the strip: it finds where its bytes differ from
//                        their predecessor (the run starts) and its share of the Adler-32 sums; the run that reaches into a piece
//                        and the next run start behind it come from the neighbours' records in LDS (a segmented scan over 256
//                        records), so a thread cuts its tokens alone.  Histogram by LDS atomics; the used symbols are ranked by
//                        all threads, ONE lane builds and limits the code lengths and the block header (png_math.h, plain C++),
//                        all threads assign the canonical codes and count the bits under both tables; the smaller block wins.
//                        Bits are packed by prefix sum: a thread stores the 32-bit words it fills alone and ORs the two it may
//                        share into the zeroed slot, at the strip's worst-case offset of the scratch.  The CRC-32 of the chunk is
//                        the XOR of the threads' pieces, each moved to its place by a multiplication modulo the CRC polynomial.
//   png_assemble_kernel  a workgroup per group of strips sums the segment sizes before its group, writes the chunk framing and
//                        moves the segments to their final offsets; the first also writes signature, IHDR and the zlib header,
//                        the last the combined Adler-32, IEND and the length word.  Every byte below the length exactly once.
// Integer arithmetic only; no host synchronisation, no allocation; the text both kernels run is png_math.h.
#include "d3ga_internal.h"
#include "png_math.h"

namespace d3ga {

static_assert(kPngThreads == kBlock, "a strip's threads are the workgroup");
static_assert(sizeof(PngShared) + kPngLdsBytes <= 65536, "a staged strip and its tables fit the default LDS limit");
constexpr int64_t kPngAssembleGroups = 1024;      // workgroups of the assembly, at most: each sums the sizes before its strips

constexpr int kPngUnroll = 8;
// bytes x0, x0 + 64, ... of a row and their neighbours (png_neighbours), every load issued before the first use; an index past
// the row is clamped into it (the caller drops that element), so nothing outside the row is read
__device__ __forceinline__ void png_load_group(const uint8_t *cur, const uint8_t *up, int64_t rb, int bpp, int64_t x0, int *v, int *a, int *b,
                                               int *c) {
#pragma unroll
    for (int u = 0; u < kPngUnroll; ++u) {
        int64_t x = x0 + 64 * u;
        if (x >= rb) x = rb - 1;
        const bool left = x >= bpp;
        const int64_t xl = left ? x - bpp : 0;
        v[u] = cur[x];
        const int av = cur[xl], bv = up ? up[x] : 0, cv = up ? up[xl] : 0;
        a[u] = left ? av : 0;
        b[u] = bv;
        c[u] = left ? cv : 0;
    }
}

__global__ __launch_bounds__(kPngThreads) void png_strip_kernel(const PngPlan p, const uint8_t *__restrict__ img, uint8_t *__restrict__ scratch) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_bytes[];
    __shared__ PngShared sh;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int64_t s = blockIdx.x;
    const int64_t rows = png_strip_rows(p, s), n = rows * (p.rb + 1);
    uint8_t *f = p.use_lds ? s_bytes : scratch + p.filt_off + s * p.n_full;
    uint32_t *slot = reinterpret_cast<uint32_t *>(scratch + p.slot_off + s * p.slot);
    png_shared_clear(sh, t);
    // filter: a wavefront per row, lanes across its bytes, kPngUnroll bytes per lane in flight (the loop is bound by load latency)
    for (int64_t r = wave; r < rows; r += kPngThreads / 64) {
        const int64_t y = s * p.rows + r;
        const uint8_t *cur = img + y * p.pitch, *up = y > 0 ? cur - p.pitch : nullptr;
        uint8_t *dst = f + r * (p.rb + 1);
        int type = p.filter;
        if (type == D3GA_PNG_FILTER_ADAPTIVE) {
            uint64_t cost[5] = {0, 0, 0, 0, 0};
            for (int64_t x0 = lane; x0 < p.rb; x0 += 64 * kPngUnroll) {
                int v[kPngUnroll], a[kPngUnroll], b[kPngUnroll], c[kPngUnroll];
                png_load_group(cur, up, p.rb, p.C, x0, v, a, b, c);
#pragma unroll
                for (int u = 0; u < kPngUnroll; ++u)
                    if (x0 + 64 * u < p.rb)
#pragma unroll
                        for (int k = 0; k < 5; ++k) cost[k] += png_abs8(png_filter_byte(k, v[u], a[u], b[u], c[u]));
            }
#pragma unroll
            for (int k = 0; k < 5; ++k)
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) cost[k] += (uint64_t)__shfl_xor((unsigned long long)cost[k], off);
            type = png_choose_filter(cost);
        }
        if (lane == 0) dst[0] = (uint8_t)type;
        for (int64_t x0 = lane; x0 < p.rb; x0 += 64 * kPngUnroll) {
            int v[kPngUnroll], a[kPngUnroll], b[kPngUnroll], c[kPngUnroll];
            png_load_group(cur, up, p.rb, p.C, x0, v, a, b, c);
#pragma unroll
            for (int u = 0; u < kPngUnroll; ++u)
                if (x0 + 64 * u < p.rb) dst[1 + x0 + 64 * u] = png_filter_byte(type, v[u], a[u], b[u], c[u]);
        }
    }
    __syncthreads();
    png_phase_breaks(sh, f, n, t);
    __syncthreads();
    png_phase_count(sh, f, n, t);
    __syncthreads();
    png_phase_sort(sh, t);
    __syncthreads();
    if (t == 0) png_phase_tables(sh);
    __syncthreads();
    png_phase_codes(sh, t);
    __syncthreads();
    const int type = png_choose_type(sh);
    if (type == kPngTypeFixed) {
        png_phase_fixed(sh, t);
        __syncthreads();
    }
    png_phase_cost(sh, f, n, type, t);
    __syncthreads();
    const uint64_t seg = png_segment_bytes(sh, type);
    for (uint64_t w = t; w < (seg + 3) / 4; w += kPngThreads) slot[w] = 0u;
    __threadfence();
    __syncthreads();
    png_phase_emit(sh, f, n, type, seg, slot, t);
    __threadfence();
    __syncthreads();
    png_phase_crc(sh, slot, seg, t);
    __syncthreads();
    if (t == 0) png_strip_meta(sh, n, seg, reinterpret_cast<uint32_t *>(scratch) + kPngMetaWords * s);
}

__global__ __launch_bounds__(kPngThreads) void png_assemble_kernel(const PngPlan p, const uint8_t *__restrict__ scratch, uint8_t *__restrict__ out,
                                                                   const int64_t per_group) {
    __shared__ uint64_t s_base, s_a, s_b;
    const int t = threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * per_group, last = first + per_group < p.S ? first + per_group : p.S;
    const bool is_last = blockIdx.x == gridDim.x - 1;
    const uint32_t *meta = reinterpret_cast<const uint32_t *>(scratch);
    if (t == 0) s_base = s_a = s_b = 0;
    __syncthreads();
    uint64_t base = 0;
    for (int64_t u = t; u < first; u += kPngThreads) base += (uint64_t)meta[kPngMetaWords * u] + 12;
    if (base) D3GA_PNG_ADD64(&s_base, base);
    if (is_last) {
        uint64_t a = 0, b = 0;
        for (int64_t u = t; u < p.S; u += kPngThreads) png_adler_terms(p, u, meta + kPngMetaWords * u, a, b);
        D3GA_PNG_ADD64(&s_a, a);
        D3GA_PNG_ADD64(&s_b, b % kPngAdlerMod);
    }
    __syncthreads();
    uint8_t *o = out + 8;
    if (blockIdx.x == 0 && t == 0) png_write_head(p, o);
    int64_t at = kPngHeadBytes + (int64_t)s_base;
    for (int64_t u = first; u < last; ++u) {
        const uint32_t *m = meta + kPngMetaWords * u;
        const uint8_t *src = scratch + p.slot_off + u * p.slot;
        const int64_t len = m[0];
        if (t == 0) {
            png_put_be32(o + at, m[0]);
            o[at + 4] = 'I'; o[at + 5] = 'D'; o[at + 6] = 'A'; o[at + 7] = 'T';
        }
        if (t == 64) png_put_be32(o + at + 8 + len, m[1]);
        for (int64_t i = t; i < len; i += kPngThreads) o[at + 8 + i] = src[i];
        at += 12 + len;
    }
    if (is_last && t == 0) {
        png_write_tail(png_adler_finish(p, s_a, s_b), o + at);
        *reinterpret_cast<uint64_t *>(out) = (uint64_t)(at + kPngTailBytes);
    }
}

}  // namespace d3ga

using namespace d3ga;

extern "C" int64_t d3ga_png_capacity(int32_t H, int32_t W, int32_t C, int32_t rows_per_strip, int64_t *scratch_bytes) {
    PngPlan p;
    const int st = png_plan_sizes(H, W, C, rows_per_strip, &p);
    if (st != D3GA_OK) return st;
    if (scratch_bytes) *scratch_bytes = p.scratch_bytes;
    return p.capacity;
}

extern "C" int d3ga_png_check(int32_t H, int32_t W, int32_t C, int64_t pitch, int32_t filter, int32_t rows_per_strip, const void *img,
                              const void *out, int64_t out_bytes, const void *scratch, int64_t scratch_bytes) {
    PngPlan p;
    return png_plan(H, W, C, pitch, filter, rows_per_strip, img, out, out_bytes, scratch, scratch_bytes, &p);
}

extern "C" int d3ga_png_encode(int32_t H, int32_t W, int32_t C, int64_t pitch, int32_t filter, int32_t rows_per_strip, const void *img, void *out,
                               int64_t out_bytes, void *scratch, int64_t scratch_bytes, d3ga_stream_t stream) {
    PngPlan p;
    D3GA_TRY(png_plan(H, W, C, pitch, filter, rows_per_strip, img, out, out_bytes, scratch, scratch_bytes, &p));
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = p.use_lds ? (size_t)((p.n_full + 15) & ~int64_t(15)) : 0;
    hipLaunchKernelGGL(png_strip_kernel, dim3((unsigned)p.S), dim3(kPngThreads), lds, s, p, (const uint8_t *)img, (uint8_t *)scratch);
    D3GA_TRY(check_launch(s, 0));
    const int64_t per_group = (p.S + kPngAssembleGroups - 1) / kPngAssembleGroups;
    const int64_t groups = (p.S + per_group - 1) / per_group;
    hipLaunchKernelGGL(png_assemble_kernel, dim3((unsigned)groups), dim3(kPngThreads), 0, s, p, (const uint8_t *)scratch, (uint8_t *)out, per_group);
    return check_launch(s, 0);
}
