// frame_prep.hip -- frame preparation: the image path of the reference's Batcher.process (lib/batch.py:141-271), once per
// training frame in front of cage_net, in ONE launch:
//   :154        fg = (seg_part > 0) | (seg_fg > 0)
//   :157        alpha = median_blur(fg, (7, 7))      kornia: zero padding, the median of 49 = the 25th smallest
//   :159-163    erode_mask (dilate 7x7, erode 5x5), close_holes (dilate 5x5, erode 5x5)   utils/image_utils.py:49-70
//   :180        orig = calibrate_color(image)        v / 255, or linear2color_corr of it (use_gamma_space)
//   :205-208    image = orig fg + (1 - fg), or orig fg (black background)
//   :236        silhouette = get_silhouette(seg_part)  a colour per label: here a table (frame_prep.py: silhouette_table)
// fg is binary, so the median is a majority vote (>= 25 of 49), a dilation "at least one" and an erosion "all of the in-image
// window": every stage is a window COUNT with a threshold (frame_prep_math.h).
//
// One workgroup (256 threads) owns a 64 x 32 tile of one image; blockIdx.z is the image.  It loads fg with a halo of 3 (+ 5 with
// erode_mask, + 4 with close_holes) rows -- and always 12 columns, so that a plane row is a constant 22 words -- into a 0 / 1
// byte plane in LDS (4.8 KB), four pixels to a word, and runs each stage as separable word sums: row counts into a second
// plane, column counts and the rule back into the first.  The valid region shrinks by the stage's radius each time and ends as
// the tile.  The tile's own fg bytes and colour-table rows are kept aside (2 + 8 KB): 20 KB of LDS in all, which leaves the
// 32 wavefronts per CU in place.  No atomics, no scratch.
//
// The eleven float planes that leave (image, orig, silhouette: 3 each; alpha: 1) and the three that enter are streamed with
// 16-byte accesses: 16 lanes per tile row, lane i at the i-th 16-byte ALIGNED quad of the row's part of the plane.  A row of
// plane q starts at element ((b C + c) H + y) W, so with W % 4 != 0 (the Goliath frame is 747 wide) the phase differs from row
// to row and from plane to plane; the pixels of a quad that hangs over the tile's left or right edge are done one by one, by
// the lane that holds the quad and, for the quad behind the sixteenth, by lane 0.  Every pixel of the tile is written exactly
// once.  The halo itself is read with coalesced 4-byte loads (two planes of the fifteen; its overlap is served by L2).
#include "d3ga_internal.h"
#include "frame_prep_math.h"

namespace d3ga {

constexpr int kFrameLanes = kFrameTileW / 4;                 // lanes per tile row
constexpr int kFrameRowsPerPass = kBlock / kFrameLanes;

// lane's share of tile row [X0, X1) of a plane row that starts at element o: vec(x) for an aligned quad inside the tile,
// one(x) for each pixel of a quad that hangs over an edge
template <class V, class O>
__device__ __forceinline__ void frame_row_quads(size_t o, int X0, int X1, int lane, V vec, O one) {
    const int p = (int)((o + (size_t)X0) & 3);
    const int xq = X0 - p + 4 * lane;
    if (xq >= X0 && xq + 4 <= X1) {
        vec(xq);
    } else {
        for (int x = max(xq, X0); x < min(xq + 4, X1); ++x) one(x);
    }
    if (lane == 0 && p)
        for (int x = X0 - p + kFrameTileW; x < X1; ++x) one(x);
}

template <bool U8>
__global__ __launch_bounds__(kBlock) void frame_prep_kernel(int H, int W, int flags, const void *__restrict__ image,
                                                            const void *__restrict__ seg_part, const float *__restrict__ seg_fg,
                                                            const float *__restrict__ label_rgb, int n_labels,
                                                            const float *__restrict__ other_rgb, float *__restrict__ image_out,
                                                            float *__restrict__ orig_out, float *__restrict__ alpha_out,
                                                            float *__restrict__ sil_out) {
    __shared__ uint32_t s_plane[kFramePlaneWords], s_cnt[kFramePlaneWords];
    __shared__ int32_t s_label[kFrameTileW * kFrameTileH];
    __shared__ uint8_t s_fg[kFrameTileW * kFrameTileH];
    const int tid = threadIdx.x;
    const int b = blockIdx.z, ty0 = blockIdx.y * kFrameTileH, tx0 = blockIdx.x * kFrameTileW;
    int halo;
    frame_tile_masks(s_plane, s_cnt, s_label, s_fg, flags, alpha_out != nullptr, b, H, W, ty0, tx0, seg_part, seg_fg, n_labels, tid,
                     kBlock, [] { __syncthreads(); }, &halo);
    const uint8_t *alpha_b = reinterpret_cast<const uint8_t *>(s_plane) + halo * kFrameCols + kFrameMaxHalo;
    const bool gamma = (flags & D3GA_FRAME_GAMMA) != 0;
    const float bg = (flags & D3GA_FRAME_BG_WHITE) ? 1.f : 0.f;
    const bool colour = image_out || orig_out;
    const int lane = tid % kFrameLanes;
    const int X1 = min(tx0 + kFrameTileW, W);
    // (no barrier below this line: rows outside the image simply leave)
    for (int ty = tid / kFrameLanes; ty < kFrameTileH; ty += kFrameRowsPerPass) {
        const int y = ty0 + ty;
        if (y >= H) break;
        const int t0 = ty * kFrameTileW - tx0;               // tile index of pixel x of this row: t0 + x
        if (colour || sil_out) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const size_t o = (((size_t)b * 3 + c) * H + y) * W;
                auto one = [&](int x) {
                    if (colour) {
                        const float v = U8 ? (float)static_cast<const uint8_t *>(image)[o + x] : static_cast<const float *>(image)[o + x];
                        const float org = frame_orig(v, c, gamma);
                        if (orig_out) orig_out[o + x] = org;
                        if (image_out) image_out[o + x] = s_fg[t0 + x] ? org : bg;
                    }
                    if (sil_out) sil_out[o + x] = frame_sil(s_label[t0 + x], c, label_rgb, n_labels, other_rgb, bg);
                };
                auto vec = [&](int x) {
                    if (colour) {
                        float v[4];
                        if (U8) {
                            const uchar4 q = *reinterpret_cast<const uchar4 *>(static_cast<const uint8_t *>(image) + o + x);
                            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
                        } else {
                            const float4 q = *reinterpret_cast<const float4 *>(static_cast<const float *>(image) + o + x);
                            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
                        }
                        float org[4], img[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            org[j] = frame_orig(v[j], c, gamma);
                            img[j] = s_fg[t0 + x + j] ? org[j] : bg;
                        }
                        if (orig_out) *reinterpret_cast<float4 *>(orig_out + o + x) = make_float4(org[0], org[1], org[2], org[3]);
                        if (image_out) *reinterpret_cast<float4 *>(image_out + o + x) = make_float4(img[0], img[1], img[2], img[3]);
                    }
                    if (sil_out) {
                        float s[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) s[j] = frame_sil(s_label[t0 + x + j], c, label_rgb, n_labels, other_rgb, bg);
                        *reinterpret_cast<float4 *>(sil_out + o + x) = make_float4(s[0], s[1], s[2], s[3]);
                    }
                };
                frame_row_quads(o, tx0, X1, lane, vec, one);
            }
        }
        if (alpha_out) {
            const size_t o = ((size_t)b * H + y) * W;
            const uint8_t *row = alpha_b + ty * kFrameCols - tx0;
            frame_row_quads(
                o, tx0, X1, lane,
                [&](int x) { *reinterpret_cast<float4 *>(alpha_out + o + x) = make_float4(row[x], row[x + 1], row[x + 2], row[x + 3]); },
                [&](int x) { alpha_out[o + x] = row[x]; });
        }
    }
}

}  // namespace d3ga

using namespace d3ga;

extern "C" int d3ga_frame_prep(int32_t B, int32_t H, int32_t W, int32_t flags, const void *image, const void *seg_part,
                               const float *seg_fg, const float *label_rgb, int32_t n_labels, const float *other_rgb,
                               float *image_out, float *orig_out, float *alpha_out, float *sil_out, d3ga_stream_t stream) {
    if (B <= 0 || H <= 0 || W <= 0 || n_labels < 1) return D3GA_E_SIZE;
    if (B > 65535 || (int64_t)H * W > INT32_MAX) return D3GA_E_SIZE;         // the grid's z extent; 32-bit pixel indices
    if (flags & ~D3GA_FRAME_ALL) return D3GA_E_CONFIG;
    if (!image || !seg_part || !label_rgb || !other_rgb) return D3GA_E_NULL;
    if (!image_out && !orig_out && !alpha_out && !sil_out) return D3GA_E_NULL;
    const uintptr_t a = (uintptr_t)image | (uintptr_t)image_out | (uintptr_t)orig_out | (uintptr_t)alpha_out | (uintptr_t)sil_out;
    if ((a & 15) || ((uintptr_t)seg_part & 3) || ((uintptr_t)seg_fg & 3)) return D3GA_E_CONFIG;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((W + kFrameTileW - 1) / kFrameTileW, (H + kFrameTileH - 1) / kFrameTileH, B);
    if (grid.y > 65535) return D3GA_E_SIZE;
    if (flags & D3GA_FRAME_IMAGE_U8)
        hipLaunchKernelGGL(frame_prep_kernel<true>, grid, dim3(kBlock), 0, s, H, W, flags, image, seg_part, seg_fg, label_rgb, n_labels,
                           other_rgb, image_out, orig_out, alpha_out, sil_out);
    else
        hipLaunchKernelGGL(frame_prep_kernel<false>, grid, dim3(kBlock), 0, s, H, W, flags, image, seg_part, seg_fg, label_rgb, n_labels,
                           other_rgb, image_out, orig_out, alpha_out, sil_out);
    return check_launch(s, 0);
}
