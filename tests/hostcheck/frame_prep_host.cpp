// CPU build of d3ga_amd/csrc/frame_prep_math.h: the tile loop of frame_prep.hip with one "thread" per tile and the header's
// own per-pixel functions and window-count stages.  Built by tests/test_frame_prep_host.py (g++ -ffp-contract=off).
#include <vector>

#include "../../d3ga_amd/csrc/frame_prep_math.h"

using namespace d3ga;

extern "C" {

void hc_frame_orig(int n, const float *v, int c, int gamma, float *out) {
    for (int i = 0; i < n; ++i) out[i] = frame_orig(v[i], c, gamma != 0);
}

// same arguments as d3ga_frame_prep (include/d3ga.h), host memory
int hc_frame_prep(int B, int H, int W, int flags, const void *image, const void *seg_part, const float *seg_fg, const float *label_rgb,
                  int n_labels, const float *other_rgb, float *image_out, float *orig_out, float *alpha_out, float *sil_out) {
    std::vector<uint32_t> plane(kFramePlaneWords), cnt(kFramePlaneWords);
    std::vector<int32_t> labels(kFrameTileW * kFrameTileH);
    std::vector<uint8_t> fg(kFrameTileW * kFrameTileH);
    const bool gamma = (flags & D3GA_FRAME_GAMMA) != 0;
    const float bg = (flags & D3GA_FRAME_BG_WHITE) ? 1.f : 0.f;
    for (int b = 0; b < B; ++b)
        for (int ty0 = 0; ty0 < H; ty0 += kFrameTileH)
            for (int tx0 = 0; tx0 < W; tx0 += kFrameTileW) {
                int halo;
                frame_tile_masks(plane.data(), cnt.data(), labels.data(), fg.data(), flags, alpha_out != nullptr, b, H, W, ty0, tx0,
                                 seg_part, seg_fg, n_labels, 0, 1, [] {}, &halo);
                const uint8_t *pb = reinterpret_cast<const uint8_t *>(plane.data());
                for (int ty = 0; ty < kFrameTileH && ty0 + ty < H; ++ty)
                    for (int tx = 0; tx < kFrameTileW && tx0 + tx < W; ++tx) {
                        const int y = ty0 + ty, x = tx0 + tx, t = ty * kFrameTileW + tx;
                        for (int c = 0; c < 3; ++c) {
                            const size_t o = (((size_t)b * 3 + c) * H + y) * W + x;
                            const float v = (flags & D3GA_FRAME_IMAGE_U8) ? (float)static_cast<const uint8_t *>(image)[o]
                                                                          : static_cast<const float *>(image)[o];
                            const float org = frame_orig(v, c, gamma);
                            if (orig_out) orig_out[o] = org;
                            if (image_out) image_out[o] = fg[t] ? org : bg;
                            if (sil_out) sil_out[o] = frame_sil(labels[t], c, label_rgb, n_labels, other_rgb, bg);
                        }
                        if (alpha_out) alpha_out[((size_t)b * H + y) * W + x] = pb[(ty + halo) * kFrameCols + tx + kFrameMaxHalo];
                    }
            }
    return 0;
}
}
