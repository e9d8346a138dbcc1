// mesh_labels_math.h -- the rules of part-label transfer onto a body mesh (mesh_labels.hip): what the
// reference's lib/segmentation.py::Segmenter.run does between the rasterizer's fragments and face_to_label.npy
// (Renderer.forward :59-74, majority_vote :112-123, utils/mesh_utils.py::median_filter_mesh :345-360), and
// lib/cage.py::grow_mask_region :131-153, restated per face.  Compiles for the host as it is:
// tests/hostcheck/mesh_labels_host.cpp runs this very text on the CPU against tests/mesh_labels_ref.py, and the kernels give
// its bytes.  Everything is integer: no rounding anywhere, so no compiler flag matters.
//
//   neighbours  (F,3) int32, -1 padded: the faces across the edges that occur in exactly two faces (built on the host).  An
//               entry outside [0, F) counts as absent everywhere below.
//   view pick   per view and face: the label at the pixel with the largest y W + x among the pixels whose pix_to_face is the
//               face (the last one in raster order); no such pixel, no vote.  pix_to_face < 0 or >= F is ignored.
//   histogram   hist (F,L) int32, L <= D3GA_LABELS_MAX: a pick with label l in [0, L) adds 1 to hist[f][l]; any other label
//               adds nothing and sets D3GA_LABEL_STATUS_RANGE in the status word.
//   majority    over labels 1 .. L-1 the largest count, ties to the smallest label; all counts 0 -> 0.
//   median      of the neighbours' labels, the face itself not among them: 1 -> that label, 2 -> (a + b) / 2 (labels are not
//               negative), 3 -> the middle one, 0 -> the face keeps its own label.
//   growth      one ring: face i qualifies when 0 < #{n in N(i): mask[n]} < #N(i), duplicates counted on both sides;
//               out[j] = mask[j] | any(i qualifies for i in N(j)).  All reads are of the ring's input mask.
#pragma once
#include <stdint.h>

#include "../../include/d3ga.h"

#ifdef __HIPCC__
#define D3GA_FHD __host__ __device__ __forceinline__
#else
#define D3GA_FHD static inline
#endif

namespace d3ga {

// a label image: pixel (b, y, x) at byte  p + b frame + y pitch + x elem, elem = 1 (uint8) or 4 (int32) bytes
struct MlImage {
    const uint8_t *p;
    int64_t pitch, frame;
    int32_t u8;
};

D3GA_FHD int32_t ml_label_at(const MlImage &im, int b, int y, int x) {
    const uint8_t *row = im.p + (int64_t)b * im.frame + (int64_t)y * im.pitch;
    return im.u8 ? (int32_t)row[x] : reinterpret_cast<const int32_t *>(row)[x];
}

struct MlVote {
    int32_t B, F, L, H, W;
    const int32_t *pix_to_face;                              // (B,H,W)
    MlImage labels;
    uint32_t *cells;                                         // (B,F): 0, or 1 + y W + x of the view's pick; all zero between calls
    int32_t *hist;                                           // (F,L)
    uint32_t *status;
};

// launch (a).  The key of a pixel; the larger key wins the cell, whatever the order of arrival.
D3GA_FHD uint32_t ml_key(int y, int x, int W) { return (uint32_t)y * (uint32_t)W + (uint32_t)x + 1u; }
D3GA_FHD bool ml_face_ok(int32_t f, int32_t F) { return (uint32_t)f < (uint32_t)F; }
// Does the pixel send its key?  `next` is the face of the pixel to its right in the same row where the same wavefront holds it
// (-1 otherwise): a pixel whose right neighbour shows the same face is dominated by it and stays silent.
D3GA_FHD bool ml_sends(int32_t f, int32_t next, int32_t F, bool suppress) { return ml_face_ok(f, F) && !(suppress && next == f); }

// launch (b): face f over the B views in order.  -> true if a label was out of range.  Leaves the face's cells at 0.
D3GA_FHD bool ml_tally_face(const MlVote &v, int f) {
    bool bad = false;
    int32_t *row = v.hist + (int64_t)f * v.L;
    for (int b = 0; b < v.B; ++b) {
        uint32_t *cell = v.cells + (int64_t)b * v.F + f;
        const uint32_t key = *cell;
        if (key == 0) continue;
        *cell = 0;
        const uint32_t pix = key - 1;
        if (pix >= (uint32_t)v.H * (uint32_t)v.W) continue;  // a cell nobody of launch (a) wrote: never read outside the image
        const int32_t l = ml_label_at(v.labels, b, (int)(pix / (uint32_t)v.W), (int)(pix % (uint32_t)v.W));
        if ((uint32_t)l < (uint32_t)v.L) row[l] += 1;
        else bad = true;
    }
    return bad;
}

D3GA_FHD int32_t ml_majority(const int32_t *row, int L) {
    int32_t best = 0, count = 0;
    for (int l = 1; l < L; ++l) {
        const int32_t c = row[l];
        if (c > count) { count = c; best = l; }
    }
    return best;
}

D3GA_FHD int ml_imin(int a, int b) { return a < b ? a : b; }
D3GA_FHD int ml_imax(int a, int b) { return a > b ? a : b; }

D3GA_FHD int32_t ml_median(const int32_t *neighbours, const int32_t *labels, int f, int F) {
    int32_t v[3];
    int k = 0;
    for (int e = 0; e < 3; ++e) {
        const int32_t n = neighbours[3 * (int64_t)f + e];
        if (ml_face_ok(n, F)) v[k++] = labels[n];
    }
    if (k == 0) return labels[f];
    if (k == 1) return v[0];
    if (k == 2) return (v[0] + v[1]) / 2;
    return ml_imax(ml_imin(v[0], v[1]), ml_imin(ml_imax(v[0], v[1]), v[2]));
}

D3GA_FHD bool ml_qualifies(const int32_t *neighbours, const uint8_t *mask, int i, int F) {
    int len = 0, in = 0;
    for (int e = 0; e < 3; ++e) {
        const int32_t n = neighbours[3 * (int64_t)i + e];
        if (!ml_face_ok(n, F)) continue;
        ++len;
        in += mask[n] != 0;
    }
    return in > 0 && in < len;
}

// one ring for face j: a two-hop pull, at most 3 + 9 + 9 reads
D3GA_FHD uint8_t ml_grow_face(const int32_t *neighbours, const uint8_t *mask, int j, int F) {
    if (mask[j]) return 1;
    for (int e = 0; e < 3; ++e) {
        const int32_t i = neighbours[3 * (int64_t)j + e];
        if (ml_face_ok(i, F) && ml_qualifies(neighbours, mask, i, F)) return 1;
    }
    return 0;
}

// ---- the argument rules of the entry points (include/d3ga.h), shared with the host build; nothing is dereferenced ---------------

static inline int ml_plan_vote(int32_t B, int32_t F, int32_t L, int32_t H, int32_t W, const int32_t *pix_to_face, const void *labels,
                               int32_t label_u8, int64_t label_pitch, int64_t label_frame, uint32_t *cells, int32_t *hist, uint32_t *status,
                               int32_t flags, MlVote *v) {
    if (B <= 0 || F <= 0 || L <= 0 || H <= 0 || W <= 0) return D3GA_E_SIZE;
    if (L > D3GA_LABELS_MAX) return D3GA_E_SIZE;
    if (B > 65535 || (int64_t)H * W >= INT32_MAX || (H + 3) / 4 > 65535) return D3GA_E_SIZE;     // the grid's z and y extents; 32-bit keys
    if ((int64_t)B * F > INT32_MAX || (int64_t)F * L > INT32_MAX) return D3GA_E_SIZE;
    if (label_u8 != 0 && label_u8 != 1) return D3GA_E_CONFIG;
    if (flags & ~D3GA_LABEL_EVERY_PIXEL) return D3GA_E_CONFIG;
    const int64_t elem = label_u8 ? 1 : 4, row = elem * W;
    if (label_pitch < row || (B > 1 && label_frame < (int64_t)(H - 1) * label_pitch + row)) return D3GA_E_CONFIG;
    if (!pix_to_face || !labels || !cells || !hist || !status) return D3GA_E_NULL;
    if (((uintptr_t)pix_to_face | (uintptr_t)cells | (uintptr_t)hist | (uintptr_t)status) & 3) return D3GA_E_CONFIG;
    if (!label_u8 && (((uintptr_t)labels | (uintptr_t)label_pitch | (uintptr_t)(B > 1 ? label_frame : 0)) & 3)) return D3GA_E_CONFIG;
    *v = {B, F, L, H, W, pix_to_face, {static_cast<const uint8_t *>(labels), label_pitch, B > 1 ? label_frame : 0, label_u8}, cells, hist, status};
    return 0;
}

static inline int ml_check_majority(int32_t F, int32_t L, const int32_t *hist, int32_t *labels) {
    if (F <= 0 || L <= 0 || L > D3GA_LABELS_MAX || (int64_t)F * L > INT32_MAX) return D3GA_E_SIZE;
    if (!hist || !labels) return D3GA_E_NULL;
    if (((uintptr_t)hist | (uintptr_t)labels) & 3) return D3GA_E_CONFIG;
    return 0;
}

static inline int ml_check_median(int32_t F, const int32_t *neighbours, const int32_t *labels, int32_t *out) {
    if (F <= 0 || (int64_t)F * 3 > INT32_MAX) return D3GA_E_SIZE;
    if (!neighbours || !labels || !out) return D3GA_E_NULL;
    if (((uintptr_t)neighbours | (uintptr_t)labels | (uintptr_t)out) & 3) return D3GA_E_CONFIG;
    if (out == labels) return D3GA_E_CONFIG;                 // every face reads its neighbours' input labels
    return 0;
}

// do the byte ranges [a, a + na) and [b, b + nb) share a byte?
static inline bool ml_overlap(const void *a, int64_t na, const void *b, int64_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + (uintptr_t)nb && y < x + (uintptr_t)na;
}

// scratch: 2 F bytes, the two masks the rings alternate between; read only with n_rings >= 2
static inline int ml_check_grow(int32_t F, int32_t n_rings, const int32_t *neighbours, const uint8_t *mask, uint8_t *out, uint8_t *scratch) {
    if (F <= 0 || (int64_t)F * 3 > INT32_MAX || n_rings < 0 || n_rings > D3GA_LABEL_RINGS_MAX) return D3GA_E_SIZE;
    if (!neighbours || !mask || !out || (n_rings >= 2 && !scratch)) return D3GA_E_NULL;
    if ((uintptr_t)neighbours & 3) return D3GA_E_CONFIG;
    if (ml_overlap(out, F, mask, F)) return D3GA_E_CONFIG;
    if (n_rings >= 2 && (ml_overlap(scratch, 2 * (int64_t)F, mask, F) || ml_overlap(scratch, 2 * (int64_t)F, out, F))) return D3GA_E_CONFIG;
    return 0;
}

// the buffer ring r of n reads and writes: mask -> s0 -> s1 -> s0 ... -> out
D3GA_FHD const uint8_t *ml_ring_src(int r, const uint8_t *mask, const uint8_t *scratch, int F) {
    return r == 0 ? mask : scratch + (int64_t)((r - 1) & 1) * F;
}
D3GA_FHD uint8_t *ml_ring_dst(int r, int n, uint8_t *out, uint8_t *scratch, int F) { return r == n - 1 ? out : scratch + (int64_t)(r & 1) * F; }

}  // namespace d3ga
