// CPU build of d3ga_amd/csrc/sample_prep_math.h: the argument rules and the per-pixel text of sample_prep.hip with one "thread"
// per pixel (path 0) or per four pixels (path 1), stored as the kernels store.  Built by tests/test_sample_prep_host.py.
#include "../../d3ga_amd/csrc/sample_prep_math.h"

using namespace d3ga;

extern "C" {

// same arguments as d3ga_sample_prep_actorshq (include/d3ga.h), host memory; force_scalar: take path 0 where the plan says 1
int hc_sample_prep_actorshq(int32_t B, int32_t H, int32_t W, int32_t Hs, int32_t Ws, const uint8_t *image, int64_t image_pitch,
                            int64_t image_frame, const uint8_t *seg, int64_t seg_pitch, int64_t seg_frame, const uint8_t *mask,
                            int64_t mask_pitch, int64_t mask_frame, int32_t mask_step, int32_t image_f32, void *image_out,
                            int32_t *seg_part_out, float *seg_fg_out, float *boundary_out, int32_t *path, int32_t force_scalar) {
    SpActors a;
    int32_t vec = 0;
    const int st = sp_plan_actorshq(B, H, W, Hs, Ws, image, image_pitch, image_frame, seg, seg_pitch, seg_frame, mask, mask_pitch, mask_frame,
                                    mask_step, image_f32, image_out, seg_part_out, seg_fg_out, boundary_out, &a, &vec);
    if (st != 0) return st;
    if (force_scalar) vec = 0;
    if (path) *path = vec;
    const size_t plane = (size_t)H * W;
    for (int b = 0; b < B; ++b)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; x += vec ? 4 : 1) {
                SpPixel p[4];
                if (vec) sp_actors_quad(a, b, y, x, p);
                else p[0] = sp_actors_pixel(a, b, y, x);
                for (int k = 0; k < (vec ? 4 : 1); ++k) {
                    const size_t o = (size_t)b * plane + (size_t)y * W + x + k, oi = 2 * (size_t)b * plane + o;
                    const uint8_t rgb[3] = {p[k].r, p[k].g, p[k].b};
                    for (int c = 0; c < 3 && image_out; ++c) {
                        if (image_f32) static_cast<float *>(image_out)[oi + c * plane] = rgb[c];
                        else static_cast<uint8_t *>(image_out)[oi + c * plane] = rgb[c];
                    }
                    if (seg_part_out) seg_part_out[o] = p[k].label;
                    if (seg_fg_out) seg_fg_out[o] = p[k].fg;
                    if (boundary_out) boundary_out[o] = p[k].boundary;
                }
            }
    return 0;
}

int hc_sample_prep_goliath(int32_t B, int32_t H, int32_t W, const uint8_t *image, int64_t image_pitch, int64_t image_plane, int64_t image_frame,
                           const uint8_t *parts, int64_t parts_pitch, int64_t parts_frame, float *image_out, float *seg_part_out,
                           float *seg_fg_out, float *boundary_out, int32_t *path) {
    SpGoliath g;
    int32_t vec = 0;
    const int st = sp_plan_goliath(B, H, W, image, image_pitch, image_plane, image_frame, parts, parts_pitch, parts_frame, image_out, seg_part_out,
                                   seg_fg_out, boundary_out, &g, &vec);
    if (st != 0) return st;
    if (path) *path = vec;
    const size_t plane = (size_t)g.oh * g.ow;
    for (int b = 0; b < B; ++b)
        for (int y = 0; y < g.oh; ++y)
            for (int x = 0; x < g.ow; ++x) {
                const SpHalf p = sp_goliath_pixel(g, b, y, x, image_out != nullptr);
                const size_t o = (size_t)b * plane + (size_t)y * g.ow + x;
                for (int c = 0; c < 3 && image_out; ++c) image_out[2 * (size_t)b * plane + o + c * plane] = p.rgb[c];
                if (seg_part_out) seg_part_out[o] = p.part;
                if (seg_fg_out) seg_fg_out[o] = p.fg;
                if (boundary_out) boundary_out[o] = 1.f - p.fg;
            }
    return 0;
}
}
