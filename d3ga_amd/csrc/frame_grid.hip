// frame_grid.hip -- the recorder's frame grid: what test.py:145-195 and train.py:344-365 do around write_text
// (utils/text_helpers.py:27-50) -- six to eight round trips of a full float image through the host for cv2.putText, th.cat into
// rows and a grid, F.pad to even sizes, and a float -> uint8 conversion with a synchronisation per written image -- as ONE
// launch per written image: labels drawn from the project's own font, panels placed, padding filled, quantised, every output
// element written exactly once.  The "{:.3f} (dB)" label reads the PSNR from its device cell, so nothing is read back.
//
// The kernel is a pure stream (4 C h w bytes per panel in, the canvas out): no LDS, no atomics.  The panel table and the label
// bytes travel in the kernel arguments, as objective.hip's pointer table does: inside a captured loop the panels are tensors of
// the graph's private pool, and a node then owns its copy of the table.  Two launch-uniform paths, chosen on the host (fg_plan):
//   vector  four horizontally adjacent pixels per thread, a 16-byte load per channel, dword / 16-byte stores -- when every
//           panel edge, pointer and pitch allows it (a group of four then never straddles a panel);
//   scalar  a pixel per thread, any strides (HWC sources, transposed and channel-sliced views), byte stores.
// Both evaluate the text of frame_grid_math.h per pixel and give the same bytes.
#include "d3ga_internal.h"
#include "frame_grid_math.h"

namespace d3ga {

// a wavefront per row segment: consecutive lanes, consecutive addresses.  64 x 4 against 256 x 1 and 16 x 16 is measured in
// DESIGN.md 4.4o (A/B builds: D3GA_VARIANT="tag:-DD3GA_GRID_BLOCK_X=256,-DD3GA_GRID_BLOCK_Y=1")
#ifndef D3GA_GRID_BLOCK_X
#define D3GA_GRID_BLOCK_X 64
#define D3GA_GRID_BLOCK_Y 4
#endif
constexpr int kGridBlockX = D3GA_GRID_BLOCK_X, kGridBlockY = D3GA_GRID_BLOCK_Y;
static_assert(kGridBlockX * kGridBlockY == 256 && kGridBlockX % 16 == 0, "256 threads, whole quarter-wavefronts per row");

__global__ __launch_bounds__(kGridBlockX *kGridBlockY) void frame_grid_scalar_kernel(const FgGrid g, void *__restrict__ out) {
    const int x = blockIdx.x * kGridBlockX + threadIdx.x, y = blockIdx.y * kGridBlockY + threadIdx.y;
    if (x >= g.out_W || y >= g.out_H) return;
    float o[4];
    fg_pixel(g, y, x, o);
    fg_store_pixel(g, out, y, x, o);
}

__device__ __forceinline__ uint32_t pack4(uint8_t a, uint8_t b, uint8_t c, uint8_t d) {
    return (uint32_t)a | ((uint32_t)b << 8) | ((uint32_t)c << 16) | ((uint32_t)d << 24);
}

__global__ __launch_bounds__(kGridBlockX *kGridBlockY) void frame_grid_vector_kernel(const FgGrid g, void *__restrict__ out) {
    const int x = 4 * (blockIdx.x * kGridBlockX + threadIdx.x), y = blockIdx.y * kGridBlockY + threadIdx.y;
    if (x >= g.out_W || y >= g.out_H) return;
    float4 R, G, B, A;
    const int i = fg_find_panel(g, y, x);
    if (i < 0) {
        R = G = B = A = make_float4(g.pad, g.pad, g.pad, g.pad);
    } else {
        const FgPanel &p = g.p[i];
        const int ly = y - p.y0, lx = x - p.x0;
        const float *s = p.src + (int64_t)ly * p.sh + lx;
        R = *reinterpret_cast<const float4 *>(s);
        G = p.C == 1 ? R : *reinterpret_cast<const float4 *>(s + p.sc);
        B = p.C == 1 ? R : *reinterpret_cast<const float4 *>(s + 2 * p.sc);
        A = p.C == 4 ? *reinterpret_cast<const float4 *>(s + 3 * p.sc) : make_float4(1.f, 1.f, 1.f, 1.f);
        const float fy = fg_row_coord(p, ly);
        if (fg_row_has_text(p, fy)) {
            const FgNum num = fg_row_number(p);
            const int numlen = fg_num_len(num);
            const float a0 = fg_alpha(p, num, numlen, fy, lx), a1 = fg_alpha(p, num, numlen, fy, lx + 1);
            const float a2 = fg_alpha(p, num, numlen, fy, lx + 2), a3 = fg_alpha(p, num, numlen, fy, lx + 3);
            R = make_float4(fg_blend(R.x, a0, p.color[0]), fg_blend(R.y, a1, p.color[0]), fg_blend(R.z, a2, p.color[0]),
                            fg_blend(R.w, a3, p.color[0]));
            G = make_float4(fg_blend(G.x, a0, p.color[1]), fg_blend(G.y, a1, p.color[1]), fg_blend(G.z, a2, p.color[1]),
                            fg_blend(G.w, a3, p.color[1]));
            B = make_float4(fg_blend(B.x, a0, p.color[2]), fg_blend(B.y, a1, p.color[2]), fg_blend(B.z, a2, p.color[2]),
                            fg_blend(B.w, a3, p.color[2]));
        }
    }
    if (g.flags & D3GA_GRID_BGR) {
        const float4 t = R;
        R = B;
        B = t;
    }
    const bool four = g.channels == 4;
    if (g.mode == D3GA_GRID_OUT_F32_CHW) {
        float *f = (float *)out + (int64_t)y * g.out_W + x;
        const int64_t plane = (int64_t)g.out_H * g.out_W;
        *reinterpret_cast<float4 *>(f) = R;
        *reinterpret_cast<float4 *>(f + plane) = G;
        *reinterpret_cast<float4 *>(f + 2 * plane) = B;
        if (four) *reinterpret_cast<float4 *>(f + 3 * plane) = A;
    } else if (g.mode == D3GA_GRID_OUT_F32_HWC) {
        float4 *f = reinterpret_cast<float4 *>((float *)out + ((int64_t)y * g.out_W + x) * g.channels);
        if (four) {
            f[0] = make_float4(R.x, G.x, B.x, A.x);
            f[1] = make_float4(R.y, G.y, B.y, A.y);
            f[2] = make_float4(R.z, G.z, B.z, A.z);
            f[3] = make_float4(R.w, G.w, B.w, A.w);
        } else {
            f[0] = make_float4(R.x, G.x, B.x, R.y);
            f[1] = make_float4(G.y, B.y, R.z, G.z);
            f[2] = make_float4(B.z, R.w, G.w, B.w);
        }
    } else {
        const int m = g.mode;
        uint32_t *w = reinterpret_cast<uint32_t *>((uint8_t *)out + (int64_t)y * g.pitch + (int64_t)x * g.channels);
        const uint8_t r0 = fg_quant(m, R.x), r1 = fg_quant(m, R.y), r2 = fg_quant(m, R.z), r3 = fg_quant(m, R.w);
        const uint8_t g0 = fg_quant(m, G.x), g1 = fg_quant(m, G.y), g2 = fg_quant(m, G.z), g3 = fg_quant(m, G.w);
        const uint8_t b0 = fg_quant(m, B.x), b1 = fg_quant(m, B.y), b2 = fg_quant(m, B.z), b3 = fg_quant(m, B.w);
        if (four) {
            w[0] = pack4(r0, g0, b0, fg_quant(m, A.x));
            w[1] = pack4(r1, g1, b1, fg_quant(m, A.y));
            w[2] = pack4(r2, g2, b2, fg_quant(m, A.z));
            w[3] = pack4(r3, g3, b3, fg_quant(m, A.w));
        } else {
            w[0] = pack4(r0, g0, b0, r1);
            w[1] = pack4(g1, b1, r2, g2);
            w[2] = pack4(b2, r3, g3, b3);
        }
    }
}

}  // namespace d3ga

using namespace d3ga;

extern "C" int d3ga_frame_grid_check(const d3ga_grid_desc *desc, const void *out, int32_t *path) {
    FgGrid g;
    return fg_plan(desc, out, &g, path);
}

extern "C" int d3ga_frame_grid(const d3ga_grid_desc *desc, void *out, int32_t *path, d3ga_stream_t stream) {
    FgGrid g;
    int32_t vec = 0;
    D3GA_TRY(fg_plan(desc, out, &g, &vec));
    if (path) *path = vec;
    hipStream_t s = (hipStream_t)stream;
    const int cols = vec ? g.out_W / 4 : g.out_W;
    const dim3 grid((unsigned)((cols + kGridBlockX - 1) / kGridBlockX), (unsigned)((g.out_H + kGridBlockY - 1) / kGridBlockY));
    if (vec) hipLaunchKernelGGL(frame_grid_vector_kernel, grid, dim3(kGridBlockX, kGridBlockY), 0, s, g, out);
    else hipLaunchKernelGGL(frame_grid_scalar_kernel, grid, dim3(kGridBlockX, kGridBlockY), 0, s, g, out);
    return check_launch(s, 0);
}
