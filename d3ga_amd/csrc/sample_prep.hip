// sample_prep.hip -- sample preparation: the numpy lines of the loader workers between the decoded files and the
// tensors of a sample (datasets/actorshq_dataset.py:244-276, get_boundary_mask :201-217; datasets/goliath_dataset.py:454-481) as
// ONE launch for B frames.  The worker hands over the uint8 arrays as imread delivers them (7 bytes per pixel instead of 18);
// what leaves is what prepare_frames, compose_target and the Evaluator take: a planar RGB image, int32 part labels and the
// float32 seg_fg and boundary_fg planes.  The rules are the text of sample_prep_math.h; this file adds the addressing only.
//
// A pure stream: no LDS, no atomics, no scratch.  The 3 x 3 window of the thresholded matte is re-read through the caches: a
// wavefront owns 64 (256 with four pixels per thread) consecutive pixels of one row and the workgroup four consecutive rows,
// so the six extra reads per pixel hit lines that the same workgroup has just fetched (a matte row of the 747-wide frame is 12
// or 36 cache lines), while the bytes that bound the launch are the 15 to 24 written per pixel.  Staging the matte in LDS would
// add a barrier and a halo fill to save reads that never reach HBM.
//
// Inputs are read byte by byte: an interleaved row of 747 pixels is 2241 bytes long, so neither a row nor a pixel is aligned to
// anything, and a dword read of the last pixel would touch bytes behind the allocation.  Outputs are planar; two launch-uniform
// paths, chosen on the host (sp_plan_*), give the same bytes:
//   vector  four horizontally adjacent pixels per thread, one 16-byte store per float32 / int32 plane row segment (a 4-byte one
//           for a uint8 image) -- when W % 4 == 0, which puts every row of every plane on that alignment;
//   scalar  a pixel per thread, element stores.
#include "d3ga_internal.h"
#include "sample_prep_math.h"

namespace d3ga {

// a wavefront per row segment, as frame_grid.hip: consecutive lanes, consecutive addresses
constexpr int kPrepBlockX = 64, kPrepBlockY = 4;
static_assert(kPrepBlockX * kPrepBlockY == kBlock, "256 threads");

template <bool F32>
__global__ __launch_bounds__(kBlock) void sample_prep_actorshq_scalar_kernel(const SpActors a) {
    const int x = blockIdx.x * kPrepBlockX + threadIdx.x, y = blockIdx.y * kPrepBlockY + threadIdx.y, b = blockIdx.z;
    if (x >= a.W || y >= a.H) return;
    const SpPixel p = sp_actors_pixel(a, b, y, x);
    const size_t plane = (size_t)a.H * a.W, o = (size_t)b * plane + (size_t)y * a.W + x;
    if (a.image_out) {
        const size_t oi = 2 * (size_t)b * plane + o;         // (b, 0, y, x) of a (B,3,H,W) tensor
        if (F32) {
            float *f = static_cast<float *>(a.image_out) + oi;
            f[0] = p.r; f[plane] = p.g; f[2 * plane] = p.b;
        } else {
            uint8_t *u = static_cast<uint8_t *>(a.image_out) + oi;
            u[0] = p.r; u[plane] = p.g; u[2 * plane] = p.b;
        }
    }
    if (a.seg_part) a.seg_part[o] = p.label;
    if (a.seg_fg) a.seg_fg[o] = p.fg;
    if (a.boundary) a.boundary[o] = p.boundary;
}

template <bool F32>
__global__ __launch_bounds__(kBlock) void sample_prep_actorshq_vector_kernel(const SpActors a) {
    const int x = 4 * (blockIdx.x * kPrepBlockX + threadIdx.x), y = blockIdx.y * kPrepBlockY + threadIdx.y, b = blockIdx.z;
    if (x >= a.W || y >= a.H) return;                        // W % 4 == 0: x + 3 < W
    SpPixel p[4];
    sp_actors_quad(a, b, y, x, p);
    const size_t plane = (size_t)a.H * a.W, o = (size_t)b * plane + (size_t)y * a.W + x;
    if (a.image_out) {
        const size_t oi = 2 * (size_t)b * plane + o;
        if (F32) {
            float *f = static_cast<float *>(a.image_out) + oi;
            *reinterpret_cast<float4 *>(f) = make_float4(p[0].r, p[1].r, p[2].r, p[3].r);
            *reinterpret_cast<float4 *>(f + plane) = make_float4(p[0].g, p[1].g, p[2].g, p[3].g);
            *reinterpret_cast<float4 *>(f + 2 * plane) = make_float4(p[0].b, p[1].b, p[2].b, p[3].b);
        } else {
            uint8_t *u = static_cast<uint8_t *>(a.image_out) + oi;
            *reinterpret_cast<uchar4 *>(u) = make_uchar4(p[0].r, p[1].r, p[2].r, p[3].r);
            *reinterpret_cast<uchar4 *>(u + plane) = make_uchar4(p[0].g, p[1].g, p[2].g, p[3].g);
            *reinterpret_cast<uchar4 *>(u + 2 * plane) = make_uchar4(p[0].b, p[1].b, p[2].b, p[3].b);
        }
    }
    if (a.seg_part) *reinterpret_cast<int4 *>(a.seg_part + o) = make_int4(p[0].label, p[1].label, p[2].label, p[3].label);
    if (a.seg_fg) *reinterpret_cast<float4 *>(a.seg_fg + o) = make_float4(p[0].fg, p[1].fg, p[2].fg, p[3].fg);
    if (a.boundary) *reinterpret_cast<float4 *>(a.boundary + o) = make_float4(p[0].boundary, p[1].boundary, p[2].boundary, p[3].boundary);
}

__global__ __launch_bounds__(kBlock) void sample_prep_goliath_scalar_kernel(const SpGoliath g) {
    const int x = blockIdx.x * kPrepBlockX + threadIdx.x, y = blockIdx.y * kPrepBlockY + threadIdx.y, b = blockIdx.z;
    if (x >= g.ow || y >= g.oh) return;
    const SpHalf p = sp_goliath_pixel(g, b, y, x, g.image_out != nullptr);
    const size_t plane = (size_t)g.oh * g.ow, o = (size_t)b * plane + (size_t)y * g.ow + x;
    if (g.image_out) {
        float *f = g.image_out + 2 * (size_t)b * plane + o;
        f[0] = p.rgb[0]; f[plane] = p.rgb[1]; f[2 * plane] = p.rgb[2];
    }
    if (g.seg_part) g.seg_part[o] = p.part;
    if (g.seg_fg) g.seg_fg[o] = p.fg;
    if (g.boundary) g.boundary[o] = 1.f - p.fg;
}

__global__ __launch_bounds__(kBlock) void sample_prep_goliath_vector_kernel(const SpGoliath g) {
    const int x = 4 * (blockIdx.x * kPrepBlockX + threadIdx.x), y = blockIdx.y * kPrepBlockY + threadIdx.y, b = blockIdx.z;
    if (x >= g.ow || y >= g.oh) return;                      // ow % 4 == 0: x + 3 < ow
    SpHalf p[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) p[k] = sp_goliath_pixel(g, b, y, x + k, g.image_out != nullptr);
    const size_t plane = (size_t)g.oh * g.ow, o = (size_t)b * plane + (size_t)y * g.ow + x;
    if (g.image_out) {
        float *f = g.image_out + 2 * (size_t)b * plane + o;
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<float4 *>(f + c * plane) = make_float4(p[0].rgb[c], p[1].rgb[c], p[2].rgb[c], p[3].rgb[c]);
    }
    if (g.seg_part) *reinterpret_cast<float4 *>(g.seg_part + o) = make_float4(p[0].part, p[1].part, p[2].part, p[3].part);
    if (g.seg_fg) *reinterpret_cast<float4 *>(g.seg_fg + o) = make_float4(p[0].fg, p[1].fg, p[2].fg, p[3].fg);
    if (g.boundary) *reinterpret_cast<float4 *>(g.boundary + o) = make_float4(1.f - p[0].fg, 1.f - p[1].fg, 1.f - p[2].fg, 1.f - p[3].fg);
}

static inline dim3 prep_grid(int H, int W, int B, int vec) {
    const int cols = vec ? W / 4 : W;
    return dim3((unsigned)((cols + kPrepBlockX - 1) / kPrepBlockX), (unsigned)((H + kPrepBlockY - 1) / kPrepBlockY), (unsigned)B);
}

}  // namespace d3ga

using namespace d3ga;

extern "C" int d3ga_sample_prep_actorshq(int32_t B, int32_t H, int32_t W, int32_t Hs, int32_t Ws, const uint8_t *image, int64_t image_pitch,
                                         int64_t image_frame, const uint8_t *seg, int64_t seg_pitch, int64_t seg_frame, const uint8_t *mask,
                                         int64_t mask_pitch, int64_t mask_frame, int32_t mask_step, int32_t image_f32, void *image_out,
                                         int32_t *seg_part_out, float *seg_fg_out, float *boundary_out, int32_t *path, d3ga_stream_t stream) {
    SpActors a;
    int32_t vec = 0;
    D3GA_TRY(sp_plan_actorshq(B, H, W, Hs, Ws, image, image_pitch, image_frame, seg, seg_pitch, seg_frame, mask, mask_pitch, mask_frame, mask_step,
                              image_f32, image_out, seg_part_out, seg_fg_out, boundary_out, &a, &vec));
    if (path) *path = vec;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid = prep_grid(H, W, B, vec), block(kPrepBlockX, kPrepBlockY);
    if (vec && image_f32) hipLaunchKernelGGL(sample_prep_actorshq_vector_kernel<true>, grid, block, 0, s, a);
    else if (vec) hipLaunchKernelGGL(sample_prep_actorshq_vector_kernel<false>, grid, block, 0, s, a);
    else if (image_f32) hipLaunchKernelGGL(sample_prep_actorshq_scalar_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(sample_prep_actorshq_scalar_kernel<false>, grid, block, 0, s, a);
    return check_launch(s, 0);
}

extern "C" int d3ga_sample_prep_goliath(int32_t B, int32_t H, int32_t W, const uint8_t *image, int64_t image_pitch, int64_t image_plane,
                                        int64_t image_frame, const uint8_t *parts, int64_t parts_pitch, int64_t parts_frame, float *image_out,
                                        float *seg_part_out, float *seg_fg_out, float *boundary_out, int32_t *path, d3ga_stream_t stream) {
    SpGoliath g;
    int32_t vec = 0;
    D3GA_TRY(sp_plan_goliath(B, H, W, image, image_pitch, image_plane, image_frame, parts, parts_pitch, parts_frame, image_out, seg_part_out,
                             seg_fg_out, boundary_out, &g, &vec));
    if (path) *path = vec;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid = prep_grid(g.oh, g.ow, B, vec), block(kPrepBlockX, kPrepBlockY);
    if (vec) hipLaunchKernelGGL(sample_prep_goliath_vector_kernel, grid, block, 0, s, g);
    else hipLaunchKernelGGL(sample_prep_goliath_scalar_kernel, grid, block, 0, s, g);
    return check_launch(s, 0);
}
