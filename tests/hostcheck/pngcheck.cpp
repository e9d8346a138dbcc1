// CPU build of d3ga_amd/csrc/png_math.h: the plan, the whole encoder run one "thread" after the other, and the code
// construction on its own.  Built by tests/png_ref.py (g++).
#include "../../d3ga_amd/csrc/png_math.h"

using namespace d3ga;

extern "C" {

// rows, strips, filtered bytes of a full strip, slot bytes, capacity, scratch bytes, staged in LDS -> status
int hc_png_plan(int32_t H, int32_t W, int32_t C, int32_t rows_per_strip, int64_t *o) {
    PngPlan p;
    const int st = png_plan_sizes(H, W, C, rows_per_strip, &p);
    if (st != D3GA_OK) return st;
    o[0] = p.rows; o[1] = p.S; o[2] = p.n_full; o[3] = p.slot; o[4] = p.capacity; o[5] = p.scratch_bytes; o[6] = p.use_lds;
    return D3GA_OK;
}

int hc_png_check(int32_t H, int32_t W, int32_t C, int64_t pitch, int32_t filter, int32_t rows_per_strip, const void *img, const void *out,
                 int64_t out_bytes, const void *scratch, int64_t scratch_bytes) {
    PngPlan p;
    return png_plan(H, W, C, pitch, filter, rows_per_strip, img, out, out_bytes, scratch, scratch_bytes, &p);
}

int hc_png_encode(int32_t H, int32_t W, int32_t C, int64_t pitch, int32_t filter, int32_t rows_per_strip, const uint8_t *img, uint8_t *out,
                  int64_t out_bytes, uint8_t *scratch, int64_t scratch_bytes, PngStripInfo *info, uint8_t *filtered) {
    return png_host_encode(H, W, C, pitch, filter, rows_per_strip, img, out, out_bytes, scratch, scratch_bytes, info, filtered);
}

// the code construction alone: freq[nsym] -> len[nsym] limited to maxbits; returns the depth of the unlimited code
int hc_png_lengths(const uint32_t *freq, int nsym, int maxbits, uint8_t *len) {
    uint16_t order[288];
    uint32_t work[288];
    int nused = 0;
    for (int s = 0; s < nsym; ++s)
        if (freq[s]) { order[png_rank(freq, nsym, s)] = (uint16_t)s; ++nused; }
    return png_lengths_sorted(freq, order, nused, nsym, maxbits, len, work);
}

// the block header of a literal/length histogram (end of block included by the caller): the lengths of both codes -> header bits
int hc_png_header(const uint32_t *freq, uint8_t *llen, uint8_t *cllen, uint32_t *clfreq, int32_t *cl_depth) {
    static PngShared sh;
    for (int t = 0; t < kPngThreads; ++t) png_shared_clear(sh, t);
    for (int s = 0; s < kPngLitLen; ++s) sh.freq[s] = freq[s];
    for (int t = 0; t < kPngThreads; ++t) png_phase_sort(sh, t);
    png_phase_tables(sh);
    for (int s = 0; s < kPngLitLen; ++s) llen[s] = sh.llen[s];
    for (int s = 0; s < kPngCl; ++s) { cllen[s] = sh.cllen[s]; clfreq[s] = sh.clfreq[s]; }
    uint8_t unl[kPngCl];
    *cl_depth = hc_png_lengths(sh.clfreq, kPngCl, kPngClMaxBits, unl);
    return (int)sh.hdr_bits;
}

uint32_t hc_png_crc(const uint8_t *p, int64_t n) { return png_crc(p, n); }
uint32_t hc_png_crc_shift(uint32_t crc, uint64_t after) { return png_crc_shift(crc, after); }
int hc_png_default_rows(int32_t H, int32_t W, int32_t C) { return (int)png_default_rows(H, W, C); }
}
