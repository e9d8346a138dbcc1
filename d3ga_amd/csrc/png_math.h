// png_math.h -- the PNG encoder of the recorder's written images (png.hip): the byte stream, the filters, the run tokens, the
// Huffman code construction and its length limiting, the bit packing and the checksums.  Semantics: DESIGN.md 4.4p
// (specification of record).  Compiles for the host as it is: tests/hostcheck/pngcheck.cpp runs this very text on the CPU, one
// "thread" after the other, and that g++ build is the yardstick -- the kernels give the same bytes.  Integer arithmetic only.
//
//   stream      signature | IHDR | IDAT "78 01" | one IDAT per strip | IDAT "03 00" + Adler-32 (big endian) | IEND.  Every chunk
//               has its own CRC-32; no CRC is combined across chunks.  Colour type 0 / 2 / 6 for C = 1 / 3 / 4, depth 8.
//   strip       rows_per_strip consecutive rows = n = rows (W C + 1) filtered bytes, one byte-aligned deflate segment:
//               ONE block (dynamic or fixed tables, whichever has fewer bits, ties to fixed) and the empty stored block
//               "00 00 FF FF" of a sync flush.  Default rows_per_strip (png_default_rows): the most rows whose filtered bytes
//               fit kPngStripTarget, at least one.  kPngStripTarget = 32 KiB is chosen by measurement: on the
//               1080p body-on-white frame one row per strip (5.6 KiB) gives a file 3.4 % larger than 45 rows (253 KiB), the
//               default's 5 rows 0.63 % larger, with 216 strips for 256 compute units and the strip staged in LDS.
//   filter      byte x of row y against a = raw[y][x - C], b = raw[y - 1][x], c = raw[y - 1][x - C], zeros outside the image
//               (the FIRST row of a strip still sees the raw row above it).  None x; Sub x - a; Up x - b; Average
//               x - ((a + b) >> 1) with the 9-bit sum; Paeth x - (pa <= pb && pa <= pc ? a : pb <= pc ? b : c).  Adaptive: the
//               type with the smallest sum of |int8(filtered)| over the row, ties to the lower type.
//   tokens      literals and matches at distance 1 (runs), lengths 3..258, as zlib's Z_RLE.  A maximal run of L equal bytes is
//               its first byte as a literal, then the other L - 1 cut greedily into matches of 258; a remainder of 3 or more
//               is one more match, of 1 or 2 is literals.  No run crosses a strip.
//   tables      literal/length code: Huffman over the strip's histogram (end-of-block counts once), limited to 15 bits;
//               distance code: the single code 0 of length 1; code-length code: Huffman limited to 7 bits.  The block header
//               DOES use symbols 16, 17 and 18, greedily, over the HLIT + 1 lengths as one sequence.
//   construction  png_rank sorts the used symbols by (count, symbol); png_lengths_sorted builds the unlimited depths in place
//               (Moffat & Katajainen 1995; where a leaf and an internal node weigh the same, the internal node is taken
//               first -- of the optimal codes the deepest) and limits them: depths beyond the limit are cut to it, and while the Kraft sum
//               exceeds one, one code of the limit is taken away and the deepest shorter code is split into two one level
//               down; the counts per length are then dealt out from the rarest symbol.  Canonical codes, by (length, symbol).
//   capacity    a literal costs at most 9 bits and a match of >= 3 bytes at most 18: a strip of n bytes needs at most
//               ceil(9 n / 8) + 8 bytes, plus 12 of chunk framing; the fixed chunks are 8 + 25 + 14 + 18 + 12 = 77 bytes:
//               png_capacity = 77 + sum over strips (ceil(9 n_s / 8) + 20).
//   limits      W C <= 2^31 - 1 and a strip of at most 2^31 - 1 filtered bytes (positions inside a strip are 32-bit).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/d3ga.h"

#ifndef D3GA_FHD
#ifdef __HIPCC__
#define D3GA_FHD __host__ __device__ __forceinline__
#else
#define D3GA_FHD static inline
#endif
#endif

// member functions of the token visitors
#ifdef __HIPCC__
#define D3GA_PNG_MEM __host__ __device__ __forceinline__
#else
#define D3GA_PNG_MEM inline
#endif

// what many "threads" of a strip do to shared words: atomics on the device, plain arithmetic in the host's thread-after-thread run
#ifdef __HIP_DEVICE_COMPILE__
#define D3GA_PNG_ADD32(p, v) atomicAdd((p), (v))
#define D3GA_PNG_ADD64(p, v) atomicAdd((unsigned long long *)(p), (unsigned long long)(v))
#define D3GA_PNG_OR32(p, v) atomicOr((p), (v))
#define D3GA_PNG_XOR32(p, v) atomicXor((p), (v))
#define D3GA_PNG_LOAD32(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)   // words other threads OR-ed into
#else
#define D3GA_PNG_ADD32(p, v) (*(p) += (v))
#define D3GA_PNG_ADD64(p, v) (*(p) += (v))
#define D3GA_PNG_OR32(p, v) (*(p) |= (v))
#define D3GA_PNG_XOR32(p, v) (*(p) ^= (v))
#define D3GA_PNG_LOAD32(p) (*(p))
#endif

namespace d3ga {

constexpr int kPngThreads = 256;                 // "threads" of a strip: the workgroup of png_strip_kernel
constexpr int64_t kPngStripTarget = 32768;       // filtered bytes of a default strip, at most (one row at least)
constexpr int64_t kPngLdsBytes = 49152;          // a strip of at most this many filtered bytes is staged in LDS (with PngShared: < 64 KiB)
constexpr int kPngLitLen = 286, kPngEob = 256, kPngCl = 19;
constexpr int kPngMaxBits = 15, kPngClMaxBits = 7;
constexpr uint32_t kPngAdlerMod = 65521u, kPngCrcPoly = 0xEDB88320u;
constexpr int64_t kPngHeadBytes = 8 + 25 + 14, kPngTailBytes = 18 + 12;   // signature, IHDR, IDAT "78 01" | last IDAT, IEND
constexpr int kPngMetaWords = 4;                 // per strip: segment bytes, CRC-32 of "IDAT" + segment, Adler s1, Adler s2

// ---- plan ---------------------------------------------------------------------------------------------------------------------
struct PngPlan {
    int32_t H, W, C, filter, rows, use_lds;
    int64_t rb;            // W C: raw bytes of a row
    int64_t pitch;         // bytes between rows of the input
    int64_t S;             // strips
    int64_t n_full;        // filtered bytes of a full strip: rows (rb + 1)
    int64_t slot;          // bytes of a strip's slot in the scratch: its worst case, rounded up to 16
    int64_t filt_off, slot_off, scratch_bytes;     // scratch: [meta S x 16 bytes][filtered bytes, unless staged in LDS][slots]
    int64_t capacity;      // PNG bytes at most
};

D3GA_FHD int64_t png_default_rows(int64_t H, int64_t W, int64_t C) {
    int64_t r = kPngStripTarget / (W * C + 1);
    if (r < 1) r = 1;
    return r < H ? r : H;
}

D3GA_FHD int64_t png_strip_rows(const PngPlan &p, int64_t s) {
    const int64_t left = (int64_t)p.H - s * p.rows;
    return left < p.rows ? left : p.rows;
}
D3GA_FHD int64_t png_strip_bytes(const PngPlan &p, int64_t s) { return png_strip_rows(p, s) * (p.rb + 1); }
D3GA_FHD int64_t png_seg_bound(int64_t n) { return (9 * n + 7) / 8 + 8; }

// sizes only (no pointer): D3GA_OK, or D3GA_E_SIZE / D3GA_E_CONFIG
D3GA_FHD int png_plan_sizes(int32_t H, int32_t W, int32_t C, int32_t rows_per_strip, PngPlan *p) {
    if (C != 1 && C != 3 && C != 4) return D3GA_E_CONFIG;
    if (H < 1 || W < 1 || rows_per_strip < 0) return D3GA_E_SIZE;
    const int64_t rb = (int64_t)W * C;
    if (rb > 0x7fffffffLL) return D3GA_E_SIZE;
    int64_t rows = rows_per_strip ? rows_per_strip : png_default_rows(H, W, C);
    if (rows > H) rows = H;
    if (rows * (rb + 1) > 0x7fffffffLL) return D3GA_E_SIZE;
    p->H = H; p->W = W; p->C = C; p->filter = D3GA_PNG_FILTER_ADAPTIVE; p->rows = (int32_t)rows;
    p->rb = rb; p->pitch = rb;
    p->S = (H + rows - 1) / rows;
    p->n_full = rows * (rb + 1);
    p->use_lds = p->n_full <= kPngLdsBytes;
    p->slot = (png_seg_bound(p->n_full) + 15) & ~int64_t(15);
    p->filt_off = (p->S * 4 * kPngMetaWords + 15) & ~int64_t(15);
    p->slot_off = p->filt_off + (p->use_lds ? 0 : ((p->S * p->n_full + 15) & ~int64_t(15)));
    p->scratch_bytes = p->slot_off + p->S * p->slot;
    const int64_t n_last = png_strip_bytes(*p, p->S - 1);
    p->capacity = kPngHeadBytes + kPngTailBytes + (p->S - 1) * (png_seg_bound(p->n_full) + 12) + png_seg_bound(n_last) + 12;
    return D3GA_OK;
}

// the argument rules of d3ga_png_encode; nothing is read through a pointer
D3GA_FHD int png_plan(int32_t H, int32_t W, int32_t C, int64_t pitch, int32_t filter, int32_t rows_per_strip, const void *img,
                      const void *out, int64_t out_bytes, const void *scratch, int64_t scratch_bytes, PngPlan *p) {
    if (!img || !out || !scratch) return D3GA_E_NULL;
    const int st = png_plan_sizes(H, W, C, rows_per_strip, p);
    if (st != D3GA_OK) return st;
    if (filter < 0 || filter > D3GA_PNG_FILTER_ADAPTIVE) return D3GA_E_CONFIG;
    if (pitch < p->rb) return D3GA_E_SIZE;
    if (((uintptr_t)out & 7) || ((uintptr_t)scratch & 15)) return D3GA_E_CONFIG;
    if (out_bytes < p->capacity || scratch_bytes < p->scratch_bytes) return D3GA_E_CAPACITY;
    p->filter = filter;
    p->pitch = pitch;
    return D3GA_OK;
}

// ---- filters ------------------------------------------------------------------------------------------------------------------
D3GA_FHD int png_paeth(int a, int b, int c) {
    const int pp = a + b - c;
    const int pa = pp > a ? pp - a : a - pp, pb = pp > b ? pp - b : b - pp, pc = pp > c ? pp - c : c - pp;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
D3GA_FHD uint8_t png_filter_byte(int type, int x, int a, int b, int c) {
    switch (type) {
    case 0: return (uint8_t)x;
    case 1: return (uint8_t)(x - a);
    case 2: return (uint8_t)(x - b);
    case 3: return (uint8_t)(x - ((a + b) >> 1));
    default: return (uint8_t)(x - png_paeth(a, b, c));
    }
}
D3GA_FHD uint32_t png_abs8(uint8_t v) { return v < 128 ? v : 256u - v; }

// the neighbours of byte x of image row y (cur, up: the raw rows; up == nullptr above the image)
D3GA_FHD void png_neighbours(const uint8_t *cur, const uint8_t *up, int64_t x, int bpp, int &a, int &b, int &c) {
    a = x >= bpp ? cur[x - bpp] : 0;
    b = up ? up[x] : 0;
    c = (up && x >= bpp) ? up[x - bpp] : 0;
}
// the five sums of |int8| over bytes x0, x0 + step, ... of a row
D3GA_FHD void png_row_costs(const uint8_t *cur, const uint8_t *up, int64_t rb, int bpp, int64_t x0, int64_t step, uint64_t cost[5]) {
    for (int k = 0; k < 5; ++k) cost[k] = 0;
    for (int64_t x = x0; x < rb; x += step) {
        int a, b, c;
        png_neighbours(cur, up, x, bpp, a, b, c);
        const int v = cur[x];
        for (int k = 0; k < 5; ++k) cost[k] += png_abs8(png_filter_byte(k, v, a, b, c));
    }
}
D3GA_FHD int png_choose_filter(const uint64_t cost[5]) {
    int best = 0;
    for (int k = 1; k < 5; ++k)
        if (cost[k] < cost[best]) best = k;
    return best;
}
// bytes x0, x0 + step, ... of the filtered row into dst[1 + x]; dst[0] (the type byte) is the caller's
D3GA_FHD void png_filter_row(int type, const uint8_t *cur, const uint8_t *up, int64_t rb, int bpp, int64_t x0, int64_t step, uint8_t *dst) {
    for (int64_t x = x0; x < rb; x += step) {
        int a, b, c;
        png_neighbours(cur, up, x, bpp, a, b, c);
        dst[1 + x] = png_filter_byte(type, cur[x], a, b, c);
    }
}

// ---- symbols ------------------------------------------------------------------------------------------------------------------
// match length 3..258 -> index 0..28 of its length symbol (257 + index), the number of extra bits and their value
D3GA_FHD int png_len_index(int len, int &ebits, int &extra) {
    const int x = len - 3;
    if (len == 258) { ebits = 0; extra = 0; return 28; }
    if (x < 8) { ebits = 0; extra = 0; return x; }
    const int e = (31 - __builtin_clz((unsigned)x)) - 2;
    ebits = e;
    extra = x & ((1 << e) - 1);
    return 4 * (e + 1) + ((x >> e) & 3);
}
D3GA_FHD int png_sym_extra_bits(int s) { return (s < 265 || s == 285) ? 0 : (s - 261) >> 2; }
D3GA_FHD int png_fixed_len(int s) { return s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8; }
D3GA_FHD uint32_t png_fixed_code(int s) {
    return s < 144 ? 0x30u + s : s < 256 ? 0x190u + (s - 144) : s < 280 ? (uint32_t)(s - 256) : 0xC0u + (s - 280);
}
D3GA_FHD uint32_t png_reverse(uint32_t code, int len) {
    uint32_t r = 0;
    for (int k = 0; k < len; ++k) r |= ((code >> k) & 1u) << (len - 1 - k);
    return r;
}

// ---- code construction --------------------------------------------------------------------------------------------------------
// position of symbol s among the used symbols ordered by (count, symbol); one symbol per "thread"
D3GA_FHD int png_rank(const uint32_t *freq, int nsym, int s) {
    const uint32_t f = freq[s];
    int r = 0;
    for (int t = 0; t < nsym; ++t) {
        const uint32_t g = freq[t];
        r += (g != 0 && (g < f || (g == f && t < s))) ? 1 : 0;
    }
    return r;
}
// order[0..nused): the used symbols by ascending (count, symbol) -> len[0..nsym) limited to maxbits, Kraft sum one for
// nused >= 2 (one used symbol gets length 1); A: nused words of work space.  Returns the depth of the unlimited code.
D3GA_FHD int png_lengths_sorted(const uint32_t *freq, const uint16_t *order, int nused, int nsym, int maxbits, uint8_t *len, uint32_t *A) {
    for (int s = 0; s < nsym; ++s) len[s] = 0;
    if (nused < 1) return 0;
    if (nused == 1) { len[order[0]] = 1; return 1; }
    const int n = nused;
    for (int i = 0; i < n; ++i) A[i] = freq[order[i]];
    // phase 1: parents in place; on equal weights the internal node before the leaf
    A[0] += A[1];
    int root = 0, leaf = 2;
    for (int next = 1; next < n - 1; ++next) {
        if (leaf >= n || A[root] <= A[leaf]) { A[next] = A[root]; A[root++] = (uint32_t)next; }
        else A[next] = A[leaf++];
        if (leaf >= n || (root < next && A[root] <= A[leaf])) { A[next] += A[root]; A[root++] = (uint32_t)next; }
        else A[next] += A[leaf++];
    }
    // phase 2: depths of the internal nodes
    A[n - 2] = 0;
    for (int next = n - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
    // phase 3: depths of the leaves, deepest first
    int avbl = 1, used = 0, dpth = 0, next = n - 1;
    root = n - 2;
    while (avbl > 0) {
        while (root >= 0 && (int)A[root] == dpth) { ++used; --root; }
        while (avbl > used) { A[next--] = (uint32_t)dpth; --avbl; }
        avbl = 2 * used;
        ++dpth;
        used = 0;
    }
    const int depth = (int)A[0];
    // the limit
    uint32_t bl[16];
    for (int l = 0; l <= maxbits; ++l) bl[l] = 0;
    for (int i = 0; i < n; ++i) bl[(int)A[i] < maxbits ? A[i] : maxbits]++;
    uint64_t total = 0;
    for (int l = 1; l <= maxbits; ++l) total += (uint64_t)bl[l] << (maxbits - l);
    while (total > (1ull << maxbits)) {
        bl[maxbits]--;
        for (int l = maxbits - 1; l >= 1; --l)
            if (bl[l]) { bl[l]--; bl[l + 1] += 2; break; }
        --total;
    }
    int i = 0;
    for (int l = maxbits; l >= 1; --l)
        for (uint32_t k = 0; k < bl[l]; ++k) len[order[i++]] = (uint8_t)l;
    return depth;
}
// the canonical code of symbol s, bit-reversed for the LSB-first stream; one symbol per "thread"
D3GA_FHD uint32_t png_canonical_code(const uint8_t *len, int nsym, int s) {
    const int l = len[s];
    if (l == 0) return 0;
    uint32_t code = 0;                 // first code of length l: sum over shorter lengths of count << (l - length)
    uint32_t below = 0;
    for (int t = 0; t < nsym; ++t) {
        const int m = len[t];
        if (m != 0 && m < l) code += 1u << (l - m);
        below += (m == l && t < s) ? 1u : 0u;
    }
    return png_reverse(code + below, l);
}

// ---- bits ---------------------------------------------------------------------------------------------------------------------
// bits into a zeroed array of 32-bit words from any bit offset: a word this writer fills alone is stored, a word it may share
// with its neighbours (its first, if it starts inside one, and its last) is OR-ed in
struct PngBits {
    uint32_t *out;
    uint64_t acc;
    int64_t word;
    int n;
    bool shared;
};
D3GA_FHD void png_bits_init(PngBits &w, uint32_t *out, uint64_t bit) {
    w.out = out; w.acc = 0; w.word = (int64_t)(bit >> 5); w.n = (int)(bit & 31); w.shared = w.n != 0;
}
D3GA_FHD void png_bits_put(PngBits &w, uint32_t v, int len) {       // len <= 16
    w.acc |= (uint64_t)v << w.n;
    w.n += len;
    if (w.n >= 32) {
        const uint32_t x = (uint32_t)w.acc;
        if (w.shared) D3GA_PNG_OR32(w.out + w.word, x);
        else w.out[w.word] = x;
        w.shared = false;
        ++w.word;
        w.acc >>= 32;
        w.n -= 32;
    }
}
D3GA_FHD void png_bits_finish(PngBits &w) {
    if (w.n > 0 && (uint32_t)w.acc != 0) D3GA_PNG_OR32(w.out + w.word, (uint32_t)w.acc);
}

// ---- checksums ----------------------------------------------------------------------------------------------------------------
D3GA_FHD uint32_t png_crc_bits(uint32_t c, uint32_t v, int nbits) {      // internal state; v's low nbits, LSB first
    c ^= v;
    for (int k = 0; k < nbits; ++k) c = (c >> 1) ^ (kPngCrcPoly & (0u - (c & 1u)));
    return c;
}
D3GA_FHD uint32_t png_crc(const uint8_t *p, int64_t n) {
    uint32_t c = 0xffffffffu;
    for (int64_t i = 0; i < n; ++i) c = png_crc_bits(c, p[i], 8);
    return ~c;
}
// the CRC-32 of bytes [lo, hi) of a little-endian word array, lo a multiple of 4
D3GA_FHD uint32_t png_crc_words(const uint32_t *w, int64_t lo, int64_t hi) {
    uint32_t c = 0xffffffffu;
    int64_t i = lo;
    for (; i + 4 <= hi; i += 4) c = png_crc_bits(c, D3GA_PNG_LOAD32(w + (i >> 2)), 32);
    if (i < hi) c = png_crc_bits(c, D3GA_PNG_LOAD32(w + (i >> 2)) & ((1u << (8 * (int)(hi - i))) - 1u), 8 * (int)(hi - i));
    return ~c;
}
// polynomials modulo the CRC polynomial, reflected: bit 31 is x^0
D3GA_FHD uint32_t png_crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int k = 0; k < 32; ++k) {
        if (a & (0x80000000u >> k)) p ^= b;
        b = (b >> 1) ^ (kPngCrcPoly & (0u - (b & 1u)));
    }
    return p;
}
D3GA_FHD uint32_t png_crc_xpow8(uint64_t nbytes) {       // x^(8 nbytes)
    uint32_t p = 0x80000000u, base = 0x00800000u;
    for (; nbytes; nbytes >>= 1) {
        if (nbytes & 1) p = png_crc_mul(base, p);
        base = png_crc_mul(base, base);
    }
    return p;
}
// CRC-32 of A followed by `after` more bytes B is  png_crc_shift(crc(A), after) ^ crc(B)
D3GA_FHD uint32_t png_crc_shift(uint32_t crc, uint64_t after) { return png_crc_mul(png_crc_xpow8(after), crc); }

// ---- a strip, "thread" by "thread" --------------------------------------------------------------------------------------------
struct PngShared {
    uint32_t freq[288];          // histogram of the literal/length symbols
    uint32_t work[288];
    uint16_t order[288];
    uint16_t lcode[288];
    uint8_t llen[288];
    uint16_t cltok[288];         // the block header's code-length tokens: symbol | extra << 8
    uint32_t clfreq[kPngCl];
    uint16_t clorder[kPngCl];
    uint16_t clcode[kPngCl];
    uint8_t cllen[kPngCl];
    int32_t first_break[kPngThreads], last_break[kPngThreads];     // -1: none in the thread's bytes
    int32_t prevb[kPngThreads], nextb[kPngThreads];
    uint64_t bits[kPngThreads];  // bits of the thread's tokens
    uint64_t s1, t1;             // sum of the bytes, sum of position x byte
    uint64_t dyn_bits, fix_bits; // the tokens and the end-of-block symbol under either code
    uint32_t nused, hlit, ncltok, hclen, hdr_bits, type, depth, crc;
    uint64_t seg_bytes;
};
constexpr int kPngTypeFixed = 1, kPngTypeDynamic = 2;

D3GA_FHD void png_thread_range(int64_t n, int t, int64_t &lo, int64_t &hi) {
    const int64_t m = (n + kPngThreads - 1) / kPngThreads;
    lo = (int64_t)t * m;
    hi = lo + m;
    if (lo > n) lo = n;
    if (hi > n) hi = n;
}

D3GA_FHD void png_shared_clear(PngShared &sh, int t) {
    for (int s = t; s < 288; s += kPngThreads) { sh.freq[s] = 0; sh.llen[s] = 0; sh.lcode[s] = 0; }
    if (t < kPngCl) sh.clfreq[t] = 0;
    if (t == 0) {
        sh.s1 = sh.t1 = sh.dyn_bits = sh.fix_bits = 0;
        sh.nused = sh.crc = 0;
        sh.freq[kPngEob] = 1;
    }
}

// phase 1: where the thread's bytes differ from their predecessor, and its share of the Adler sums
D3GA_FHD void png_phase_breaks(PngShared &sh, const uint8_t *f, int64_t n, int t) {
    int64_t lo, hi;
    png_thread_range(n, t, lo, hi);
    int32_t first = -1, last = -1;
    uint64_t s1 = 0, t1 = 0;
    for (int64_t i = lo; i < hi; ++i) {
        const uint32_t v = f[i];
        if (i == 0 || f[i - 1] != v) {
            if (first < 0) first = (int32_t)i;
            last = (int32_t)i;
        }
        s1 += v;
        t1 += (uint64_t)i * v;
    }
    sh.first_break[t] = first;
    sh.last_break[t] = last;
    if (s1) { D3GA_PNG_ADD64(&sh.s1, s1); D3GA_PNG_ADD64(&sh.t1, t1); }
}

// the tokens whose first byte lies in [lo, hi): prevb = start of the run that holds byte lo, nextb = the first run start >= hi (or n)
template <class F>
D3GA_FHD void png_walk(const uint8_t *f, int64_t lo, int64_t hi, int64_t prevb, int64_t nextb, F &fn) {
    int64_t i = lo;
    while (i < hi) {
        const int64_t p = i == lo ? prevb : i;
        int64_t e = i + 1;
        while (e < hi && f[e] == f[e - 1]) ++e;
        const int64_t xe = e;
        if (e == hi) e = nextb;
        if (p == i) fn.lit(f[p]);
        const int64_t R = e - p - 1;                  // bytes of the run behind its first
        if (R > 0) {
            const int64_t s0 = i > p + 1 ? i : p + 1;
            for (int64_t q = (int64_t)((uint32_t)(s0 - (p + 1)) / 258u);; ++q) {
                const int64_t s = p + 1 + 258 * q;
                if (s >= xe) break;
                const int64_t cl = R - 258 * q < 258 ? R - 258 * q : 258;
                if (cl >= 3) {
                    if (s >= i) fn.match((int)cl);
                } else {
                    for (int64_t x = s > i ? s : i; x < s + cl && x < xe; ++x) fn.lit(f[x]);
                }
            }
        }
        i = xe;
    }
}

struct PngCount {
    uint32_t *freq;
    D3GA_PNG_MEM void lit(uint8_t v) { D3GA_PNG_ADD32(freq + v, 1u); }
    D3GA_PNG_MEM void match(int len) {
        int eb, ex;
        D3GA_PNG_ADD32(freq + 257 + png_len_index(len, eb, ex), 1u);
    }
};
struct PngCost {
    const uint8_t *llen;
    uint32_t dist_bits;
    uint64_t bits;
    D3GA_PNG_MEM void lit(uint8_t v) { bits += llen[v]; }
    D3GA_PNG_MEM void match(int len) {
        int eb, ex;
        bits += llen[257 + png_len_index(len, eb, ex)] + eb + dist_bits;
    }
};
struct PngEmit {
    const uint8_t *llen;
    const uint16_t *lcode;
    int dist_bits;
    PngBits w;
    D3GA_PNG_MEM void lit(uint8_t v) { png_bits_put(w, lcode[v], llen[v]); }
    D3GA_PNG_MEM void match(int len) {
        int eb, ex;
        const int s = 257 + png_len_index(len, eb, ex);
        png_bits_put(w, lcode[s], llen[s]);
        if (eb) png_bits_put(w, (uint32_t)ex, eb);
        png_bits_put(w, 0u, dist_bits);            // distance 1: code 0 of the one-code table (1 bit) | of the fixed table (5 bits)
    }
};

// phase 2: the run that reaches into the thread's bytes, the next run start behind them, and the histogram
D3GA_FHD void png_phase_count(PngShared &sh, const uint8_t *f, int64_t n, int t) {
    int64_t lo, hi;
    png_thread_range(n, t, lo, hi);
    if (lo >= hi) return;
    int64_t prevb = lo, nextb = n;
    if (lo > 0 && f[lo] == f[lo - 1])
        for (int u = t - 1; u >= 0; --u)
            if (sh.last_break[u] >= 0) { prevb = sh.last_break[u]; break; }
    for (int u = t + 1; u < kPngThreads; ++u)
        if (sh.first_break[u] >= 0) { nextb = sh.first_break[u]; break; }
    sh.prevb[t] = (int32_t)prevb;
    sh.nextb[t] = (int32_t)nextb;
    PngCount fn{sh.freq};
    png_walk(f, lo, hi, prevb, nextb, fn);
}

// phase 3a: the used symbols in order; symbols t and t + 256
D3GA_FHD void png_phase_sort(PngShared &sh, int t) {
    for (int s = t; s < kPngLitLen; s += kPngThreads)
        if (sh.freq[s]) {
            sh.order[png_rank(sh.freq, kPngLitLen, s)] = (uint16_t)s;
            D3GA_PNG_ADD32(&sh.nused, 1u);
        }
}

D3GA_FHD void png_cl_token(PngShared &sh, int sym, int extra) {
    sh.cltok[sh.ncltok++] = (uint16_t)(sym | (extra << 8));
    sh.clfreq[sym]++;
}
D3GA_FHD int png_cl_extra_bits(int sym) { return sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0; }
// the order in which the block header lists the lengths of the code-length code
D3GA_FHD int png_cl_order(int k) {
    switch (k) {
    case 0: return 16; case 1: return 17; case 2: return 18; case 3: return 0; case 4: return 8; case 5: return 7; case 6: return 9;
    case 7: return 6; case 8: return 10; case 9: return 5; case 10: return 11; case 11: return 4; case 12: return 12; case 13: return 3;
    case 14: return 13; case 15: return 2; case 16: return 14; case 17: return 1; default: return 15;
    }
}

// phase 3b, ONE thread: the literal/length lengths, the block header's tokens and the code-length code
D3GA_FHD void png_phase_tables(PngShared &sh) {
    sh.depth = (uint32_t)png_lengths_sorted(sh.freq, sh.order, (int)sh.nused, kPngLitLen, kPngMaxBits, sh.llen, sh.work);
    int hlit = kPngLitLen;
    while (hlit > 257 && sh.llen[hlit - 1] == 0) --hlit;
    sh.hlit = (uint32_t)hlit;
    // the lengths of hlit literal/length codes and of the one distance code (length 1), as one sequence
    sh.ncltok = 0;
    const int total = hlit + 1;
    int i = 0;
    while (i < total) {
        const int v = i < hlit ? sh.llen[i] : 1;
        int run = 1;
        while (i + run < total && (i + run < hlit ? sh.llen[i + run] : 1) == v) ++run;
        i += run;
        if (v == 0) {
            while (run >= 11) { const int r = run < 138 ? run : 138; png_cl_token(sh, 18, r - 11); run -= r; }
            if (run >= 3) { png_cl_token(sh, 17, run - 3); run = 0; }
        } else {
            png_cl_token(sh, v, 0);
            --run;
            while (run >= 3) { const int r = run < 6 ? run : 6; png_cl_token(sh, 16, r - 3); run -= r; }
        }
        for (; run > 0; --run) png_cl_token(sh, v, 0);
    }
    // the code-length code: 19 symbols, sorted here
    int nused = 0;
    for (int s = 0; s < kPngCl; ++s)
        if (sh.clfreq[s]) { sh.clorder[png_rank(sh.clfreq, kPngCl, s)] = (uint16_t)s; ++nused; }
    png_lengths_sorted(sh.clfreq, sh.clorder, nused, kPngCl, kPngClMaxBits, sh.cllen, sh.work);
    for (int s = 0; s < kPngCl; ++s) sh.clcode[s] = (uint16_t)png_canonical_code(sh.cllen, kPngCl, s);
    int hclen = kPngCl;
    while (hclen > 4 && sh.cllen[png_cl_order(hclen - 1)] == 0) --hclen;
    sh.hclen = (uint32_t)hclen;
    uint32_t bits = 3 + 5 + 5 + 4 + 3 * (uint32_t)hclen;
    for (int s = 0; s < kPngCl; ++s) bits += sh.clfreq[s] * (uint32_t)(sh.cllen[s] + png_cl_extra_bits(s));
    sh.hdr_bits = bits;
}

// phase 3c: the dynamic code of symbols t and t + 256, and what the tokens cost under either table
D3GA_FHD void png_phase_codes(PngShared &sh, int t) {
    uint64_t dyn = 0, fix = 0;
    for (int s = t; s < kPngLitLen; s += kPngThreads) {
        sh.lcode[s] = (uint16_t)png_canonical_code(sh.llen, kPngLitLen, s);
        const uint64_t f = sh.freq[s];
        if (f) {
            const int eb = png_sym_extra_bits(s);
            dyn += f * (uint64_t)(sh.llen[s] + eb + (s > 256 ? 1 : 0));
            fix += f * (uint64_t)(png_fixed_len(s) + eb + (s > 256 ? 5 : 0));
        }
    }
    if (dyn) { D3GA_PNG_ADD64(&sh.dyn_bits, dyn); D3GA_PNG_ADD64(&sh.fix_bits, fix); }
}
// the choice (every thread computes the same): ties to the fixed block
D3GA_FHD int png_choose_type(const PngShared &sh) { return sh.hdr_bits + sh.dyn_bits < 3 + sh.fix_bits ? kPngTypeDynamic : kPngTypeFixed; }
// phase 3d, after the choice: the fixed table replaces the dynamic one
D3GA_FHD void png_phase_fixed(PngShared &sh, int t) {
    for (int s = t; s < 288; s += kPngThreads) {
        sh.llen[s] = (uint8_t)png_fixed_len(s);
        sh.lcode[s] = (uint16_t)png_reverse(png_fixed_code(s), png_fixed_len(s));
    }
}

// phase 4: bits of the thread's tokens
D3GA_FHD void png_phase_cost(PngShared &sh, const uint8_t *f, int64_t n, int type, int t) {
    int64_t lo, hi;
    png_thread_range(n, t, lo, hi);
    PngCost fn{sh.llen, type == kPngTypeDynamic ? 1u : 5u, 0};
    if (lo < hi) png_walk(f, lo, hi, sh.prevb[t], sh.nextb[t], fn);
    sh.bits[t] = fn.bits;
}
D3GA_FHD uint64_t png_head_bits(const PngShared &sh, int type) { return type == kPngTypeDynamic ? sh.hdr_bits : 3; }
// bytes of the segment: block, the three header bits of the stored block, padding, 00 00 FF FF
D3GA_FHD uint64_t png_segment_bytes(const PngShared &sh, int type) {
    uint64_t bits = png_head_bits(sh, type) + sh.llen[kPngEob] + 3;
    for (int t = 0; t < kPngThreads; ++t) bits += sh.bits[t];
    return (bits + 7) / 8 + 4;
}

// phase 5: the thread's tokens into the zeroed slot; thread 0 the block header; the last thread the end of block and FF FF
D3GA_FHD void png_phase_emit(PngShared &sh, const uint8_t *f, int64_t n, int type, uint64_t seg_bytes, uint32_t *slot, int t) {
    int64_t lo, hi;
    png_thread_range(n, t, lo, hi);
    uint64_t bit = png_head_bits(sh, type);
    for (int u = 0; u < t; ++u) bit += sh.bits[u];
    PngEmit fn{sh.llen, sh.lcode, type == kPngTypeDynamic ? 1 : 5, {}};
    png_bits_init(fn.w, slot, bit);
    if (lo < hi) png_walk(f, lo, hi, sh.prevb[t], sh.nextb[t], fn);
    if (t == kPngThreads - 1) png_bits_put(fn.w, sh.lcode[kPngEob], sh.llen[kPngEob]);
    png_bits_finish(fn.w);
    if (t == kPngThreads - 1) {
        const uint64_t b = seg_bytes - 2;          // FF FF: the last two bytes
        D3GA_PNG_OR32(slot + (b >> 2), 0xffu << (8 * (b & 3)));
        D3GA_PNG_OR32(slot + ((b + 1) >> 2), 0xffu << (8 * ((b + 1) & 3)));
    }
    if (t == 0) {
        PngBits w;
        png_bits_init(w, slot, 0);
        if (type == kPngTypeFixed) {
            png_bits_put(w, 2u, 3);                // BFINAL 0, BTYPE 01
        } else {
            png_bits_put(w, 4u, 3);                // BFINAL 0, BTYPE 10
            png_bits_put(w, sh.hlit - 257, 5);
            png_bits_put(w, 0u, 5);                // HDIST - 1
            png_bits_put(w, sh.hclen - 4, 4);
            for (uint32_t k = 0; k < sh.hclen; ++k) png_bits_put(w, sh.cllen[png_cl_order((int)k)], 3);
            for (uint32_t k = 0; k < sh.ncltok; ++k) {
                const int sym = sh.cltok[k] & 31, extra = sh.cltok[k] >> 8;
                png_bits_put(w, sh.clcode[sym], sh.cllen[sym]);
                if (png_cl_extra_bits(sym)) png_bits_put(w, (uint32_t)extra, png_cl_extra_bits(sym));
            }
        }
        png_bits_finish(w);
    }
}

// phase 6: CRC-32 of "IDAT" + segment; each thread its piece of whole words, moved to its place in the message
D3GA_FHD void png_phase_crc(PngShared &sh, const uint32_t *slot, uint64_t seg_bytes, int t) {
    const uint64_t words = (seg_bytes + 3) / 4, per = 4 * ((words + kPngThreads - 1) / kPngThreads);
    const uint64_t lo = per * t < seg_bytes ? per * t : seg_bytes, hi = lo + per < seg_bytes ? lo + per : seg_bytes;
    if (lo < hi) D3GA_PNG_XOR32(&sh.crc, png_crc_shift(png_crc_words(slot, (int64_t)lo, (int64_t)hi), seg_bytes - hi));
    if (t == 0) {
        const uint8_t name[4] = {'I', 'D', 'A', 'T'};
        D3GA_PNG_XOR32(&sh.crc, png_crc_shift(png_crc(name, 4), seg_bytes));
    }
}

// what a strip leaves for the assembly: segment bytes, its chunk's CRC, and its Adler sums s1 = sum d, s2 = sum (n - i) d_i
D3GA_FHD void png_strip_meta(const PngShared &sh, int64_t n, uint64_t seg_bytes, uint32_t *meta) {
    const uint64_t M = kPngAdlerMod;
    const uint64_t s1 = sh.s1 % M;
    meta[0] = (uint32_t)seg_bytes;
    meta[1] = sh.crc;
    meta[2] = (uint32_t)s1;
    meta[3] = (uint32_t)((((uint64_t)n % M) * s1 + M - sh.t1 % M) % M);
}

// ---- assembly -----------------------------------------------------------------------------------------------------------------
D3GA_FHD void png_put_be32(uint8_t *p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v;
}
// signature, IHDR and the IDAT of the zlib header: kPngHeadBytes bytes
D3GA_FHD void png_write_head(const PngPlan &p, uint8_t *o) {
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    for (int k = 0; k < 8; ++k) o[k] = sig[k];
    uint8_t *h = o + 8;
    png_put_be32(h, 13);
    h[4] = 'I'; h[5] = 'H'; h[6] = 'D'; h[7] = 'R';
    png_put_be32(h + 8, (uint32_t)p.W);
    png_put_be32(h + 12, (uint32_t)p.H);
    h[16] = 8;
    h[17] = p.C == 1 ? 0 : p.C == 3 ? 2 : 6;
    h[18] = h[19] = h[20] = 0;
    png_put_be32(h + 21, png_crc(h + 4, 17));
    uint8_t *z = o + 33;
    png_put_be32(z, 2);
    z[4] = 'I'; z[5] = 'D'; z[6] = 'A'; z[7] = 'T'; z[8] = 0x78; z[9] = 0x01;
    png_put_be32(z + 10, png_crc(z + 4, 6));
}
// the IDAT of the final empty block and the Adler-32, and IEND: kPngTailBytes bytes
D3GA_FHD void png_write_tail(uint32_t adler, uint8_t *o) {
    png_put_be32(o, 6);
    o[4] = 'I'; o[5] = 'D'; o[6] = 'A'; o[7] = 'T'; o[8] = 0x03; o[9] = 0x00;
    png_put_be32(o + 10, adler);
    png_put_be32(o + 14, png_crc(o + 4, 10));
    uint8_t *e = o + 18;
    png_put_be32(e, 0);
    e[4] = 'I'; e[5] = 'E'; e[6] = 'N'; e[7] = 'D';
    png_put_be32(e + 8, png_crc(e + 4, 4));
}
// strip s's terms of the combined Adler-32: a = 1 + sum s1, b = N + sum (s2 + s1 x bytes behind the strip), both mod 65521
D3GA_FHD void png_adler_terms(const PngPlan &p, int64_t s, const uint32_t *meta, uint64_t &a, uint64_t &b) {
    const uint64_t total = (uint64_t)p.H * (uint64_t)(p.rb + 1);
    const uint64_t end = s + 1 < p.S ? (uint64_t)(s + 1) * (uint64_t)p.n_full : total;
    a += meta[2];
    b += meta[3] + (uint64_t)meta[2] * ((total - end) % kPngAdlerMod);
}
D3GA_FHD uint32_t png_adler_finish(const PngPlan &p, uint64_t a, uint64_t b) {
    const uint64_t total = (uint64_t)p.H * (uint64_t)(p.rb + 1);
    return (uint32_t)(((total % kPngAdlerMod + b % kPngAdlerMod) % kPngAdlerMod) << 16 | (1 + a % kPngAdlerMod) % kPngAdlerMod);
}

#ifndef __HIP_DEVICE_COMPILE__
// ---- the whole encoder on the host: the kernels' phases, one "thread" after the other -------------------------------------------
struct PngStripInfo {
    int32_t type, depth, hlit, hclen, nused;
    uint64_t dyn_bits, fix_bits, hdr_bits, seg_bytes;
    uint8_t llen[288], cllen[kPngCl];
};

static inline void png_host_filter_strip(const PngPlan &p, const uint8_t *img, int64_t s, uint8_t *f) {
    const int64_t rows = png_strip_rows(p, s);
    for (int64_t r = 0; r < rows; ++r) {
        const int64_t y = s * p.rows + r;
        const uint8_t *cur = img + y * p.pitch, *up = y > 0 ? cur - p.pitch : nullptr;
        int type = p.filter;
        if (type == D3GA_PNG_FILTER_ADAPTIVE) {
            uint64_t cost[5];
            png_row_costs(cur, up, p.rb, p.C, 0, 1, cost);
            type = png_choose_filter(cost);
        }
        uint8_t *dst = f + r * (p.rb + 1);
        dst[0] = (uint8_t)type;
        png_filter_row(type, cur, up, p.rb, p.C, 0, 1, dst);
    }
}

// filtered bytes f[0..n) -> the segment in the zeroed slot, meta[4]
static inline void png_host_strip(const uint8_t *f, int64_t n, uint32_t *slot, int64_t slot_bytes, uint32_t *meta, PngStripInfo *info) {
    static PngShared sh;
    const int T = kPngThreads;
    for (int t = 0; t < T; ++t) png_shared_clear(sh, t);
    for (int t = 0; t < T; ++t) png_phase_breaks(sh, f, n, t);
    for (int t = 0; t < T; ++t) png_phase_count(sh, f, n, t);
    for (int t = 0; t < T; ++t) png_phase_sort(sh, t);
    png_phase_tables(sh);
    for (int t = 0; t < T; ++t) png_phase_codes(sh, t);
    const int type = png_choose_type(sh);
    if (info) {
        info->type = type; info->depth = (int32_t)sh.depth; info->hlit = (int32_t)sh.hlit; info->hclen = (int32_t)sh.hclen;
        info->nused = (int32_t)sh.nused;
        info->dyn_bits = sh.hdr_bits + sh.dyn_bits; info->fix_bits = 3 + sh.fix_bits; info->hdr_bits = sh.hdr_bits;
        memcpy(info->llen, sh.llen, 288);
        memcpy(info->cllen, sh.cllen, kPngCl);
    }
    if (type == kPngTypeFixed)
        for (int t = 0; t < T; ++t) png_phase_fixed(sh, t);
    for (int t = 0; t < T; ++t) png_phase_cost(sh, f, n, type, t);
    const uint64_t seg = png_segment_bytes(sh, type);
    if (info) info->seg_bytes = seg;
    memset(slot, 0, (size_t)slot_bytes);
    for (int t = 0; t < T; ++t) png_phase_emit(sh, f, n, type, seg, slot, t);
    for (int t = 0; t < T; ++t) png_phase_crc(sh, slot, seg, t);
    png_strip_meta(sh, n, seg, meta);
}

// d3ga_png_encode on the CPU: out = [uint64 length][PNG bytes], scratch as the plan lays it out; info: S records or nullptr.
// filtered: all filtered bytes, H (rb + 1) of them, or nullptr.
static inline int png_host_encode(int32_t H, int32_t W, int32_t C, int64_t pitch, int32_t filter, int32_t rows_per_strip, const uint8_t *img,
                                  uint8_t *out, int64_t out_bytes, uint8_t *scratch, int64_t scratch_bytes, PngStripInfo *info,
                                  uint8_t *filtered) {
    PngPlan p;
    const int st = png_plan(H, W, C, pitch, filter, rows_per_strip, img, out, out_bytes, scratch, scratch_bytes, &p);
    if (st != D3GA_OK) return st;
    uint32_t *meta = (uint32_t *)scratch;
    uint8_t *f = new uint8_t[(size_t)p.n_full];
    for (int64_t s = 0; s < p.S; ++s) {
        const int64_t n = png_strip_bytes(p, s);
        png_host_filter_strip(p, img, s, f);
        if (filtered) memcpy(filtered + s * p.n_full, f, (size_t)n);
        png_host_strip(f, n, (uint32_t *)(scratch + p.slot_off + s * p.slot), p.slot, meta + kPngMetaWords * s, info ? info + s : nullptr);
    }
    delete[] f;
    uint8_t *o = out + 8;
    png_write_head(p, o);
    int64_t at = kPngHeadBytes;
    uint64_t a = 0, b = 0;
    for (int64_t s = 0; s < p.S; ++s) {
        const uint32_t *m = meta + kPngMetaWords * s;
        const uint8_t *src = scratch + p.slot_off + s * p.slot;
        png_put_be32(o + at, m[0]);
        o[at + 4] = 'I'; o[at + 5] = 'D'; o[at + 6] = 'A'; o[at + 7] = 'T';
        memcpy(o + at + 8, src, m[0]);
        png_put_be32(o + at + 8 + m[0], m[1]);
        at += 12 + (int64_t)m[0];
        png_adler_terms(p, s, m, a, b);
    }
    png_write_tail(png_adler_finish(p, a, b), o + at);
    at += kPngTailBytes;
    const uint64_t len = (uint64_t)at;
    memcpy(out, &len, 8);
    return D3GA_OK;
}
#endif

}  // namespace d3ga
