// CPU build of d3ga_amd/csrc/mesh_labels_math.h: the argument rules and the per-pixel / per-face text of mesh_labels.hip.  The
// first vote launch is walked as the kernel walks it -- rows cut into wavefronts of 64 pixels, a lane seeing the face of the
// next lane -- so the run suppression is the one the GPU applies.  Built by
// tests/mesh_labels_ref.py.
#include "../../d3ga_amd/csrc/mesh_labels_math.h"

using namespace d3ga;

extern "C" {

// same arguments as d3ga_label_vote (include/d3ga.h), host memory; *sent (may be NULL): the keys the first launch sent
int hc_label_vote(int32_t B, int32_t F, int32_t L, int32_t H, int32_t W, const int32_t *pix_to_face, const void *labels, int32_t label_u8,
                  int64_t label_pitch, int64_t label_frame, uint32_t *cells, int32_t *hist, uint32_t *status, int32_t flags, int64_t *sent) {
    MlVote v;
    const int st = ml_plan_vote(B, F, L, H, W, pix_to_face, labels, label_u8, label_pitch, label_frame, cells, hist, status, flags, &v);
    if (st != 0) return st;
    const int span = 64;
    const bool suppress = !(flags & D3GA_LABEL_EVERY_PIXEL);
    int64_t n_sent = 0;
    for (int b = 0; b < B; ++b)
        for (int y = 0; y < H; ++y) {
            const int32_t *row = pix_to_face + ((size_t)b * H + y) * W;
            for (int x = 0; x < W; ++x) {
                const bool last_of_wave = x % span == span - 1 || x == W - 1;      // lane 63's last pixel, or the row's
                const int32_t next = last_of_wave ? -1 : row[x + 1];
                if (!ml_sends(row[x], next, F, suppress)) continue;
                uint32_t *cell = cells + (size_t)b * F + row[x];
                const uint32_t key = ml_key(y, x, W);
                if (key > *cell) *cell = key;
                ++n_sent;
            }
        }
    if (sent) *sent = n_sent;
    for (int f = 0; f < F; ++f)
        if (ml_tally_face(v, f)) *status |= D3GA_LABEL_STATUS_RANGE;
    return 0;
}

int hc_label_majority(int32_t F, int32_t L, const int32_t *hist, int32_t *labels) {
    const int st = ml_check_majority(F, L, hist, labels);
    if (st != 0) return st;
    for (int f = 0; f < F; ++f) labels[f] = ml_majority(hist + (size_t)f * L, L);
    return 0;
}

int hc_label_median(int32_t F, const int32_t *neighbours, const int32_t *labels, int32_t *out) {
    const int st = ml_check_median(F, neighbours, labels, out);
    if (st != 0) return st;
    for (int f = 0; f < F; ++f) out[f] = ml_median(neighbours, labels, f, F);
    return 0;
}

int hc_label_grow(int32_t F, int32_t n_rings, const int32_t *neighbours, const uint8_t *mask, uint8_t *out, uint8_t *scratch) {
    const int st = ml_check_grow(F, n_rings, neighbours, mask, out, scratch);
    if (st != 0) return st;
    if (n_rings == 0)
        for (int j = 0; j < F; ++j) out[j] = mask[j] != 0;
    for (int r = 0; r < n_rings; ++r) {
        const uint8_t *src = ml_ring_src(r, mask, scratch, F);
        uint8_t *dst = ml_ring_dst(r, n_rings, out, scratch, F);
        for (int j = 0; j < F; ++j) dst[j] = ml_grow_face(neighbours, src, j, F);
    }
    return 0;
}
}
