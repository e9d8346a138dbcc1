// perceptual_math.h -- index maps of the VGG perceptual loss (perceptual.hip), host-compilable: the level plan, the
// K ordering of the 3x3 convolution's implicit GEMM and the layout of its packed weight panels.  The g++ build in
// tests/hostcheck/perceptual_check.cpp walks every slot of both panels against the forward map below.
//
// Implicit GEMM of a 3x3, stride-1, pad-1 convolution over channels-last activations X (H, W, Cin):
//     Y[p][n] = sum_k A[p][k] B[k][n],   p = y W + x,   n = output channel,
//     k = 8 u + j with unit u = tap Cu + c8, Cu = ceil(Cin / 8), tap = 3 ky + kx, input channel ci = 8 c8 + j,
//     A[p][k] = X[y + ky - 1][x + kx - 1][ci]  (0 outside the image or past Cin),  B[k][n] = W[n][ci][ky][kx].
// A unit is 8 consecutive channels of ONE pixel: 32 contiguous bytes, the 8 k one lane feeds v_mfma_f32_32x32x16_bf16.
// A k-step of the MFMA is two units (k-half 0 and 1); an odd unit count leaves a zero half at the end.
//
// Panel (one per direction, three bf16 planes of it): 16-byte slots of 8 bf16,
//     slot(u, n) = (u NB + n / 32) 32 + n % 32,   NB = ceil(Cout / 32),   u < 2 KK,   KK = ceil(9 Cu / 2),
// element j of the slot = piece of B[8 u + j][n]; zero where u >= 9 Cu, ci >= Cin or n >= Cout.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PC_HD __host__ __device__ inline
#else
#define PC_HD inline
#endif

namespace d3ga {

constexpr int kVggConvs = 13;       // conv1_1 .. conv5_1
constexpr int kVggTaps = 5;         // relu1_1, relu2_1, relu3_1, relu4_1, relu5_1
constexpr int kVggPlanes = 3;       // bf16 pieces per f32 weight (a later reduced-precision split would pack fewer)

PC_HD int pc_units_per_tap(int cin) { return (cin + 7) / 8; }
PC_HD int pc_units(int cin) { return 9 * pc_units_per_tap(cin); }
PC_HD int pc_ksteps(int cin) { return (pc_units(cin) + 1) / 2; }
PC_HD int pc_nblocks(int cout) { return (cout + 31) / 32; }
// 16-byte slots of ONE plane
PC_HD int64_t pc_plane_slots(int cin, int cout) { return (int64_t)pc_ksteps(cin) * 2 * pc_nblocks(cout) * 32; }
PC_HD int64_t pc_panel_bytes(int cin, int cout) { return kVggPlanes * pc_plane_slots(cin, cout) * 16; }

// Forward map: bf16 element index, within a plane, of B[k(ci, ky, kx)][n] for a GEMM with `cin` inputs and `cout` outputs.
PC_HD int64_t pc_panel_elem(int cin, int cout, int n, int ci, int ky, int kx) {
    const int u = (3 * ky + kx) * pc_units_per_tap(cin) + ci / 8;
    return (((int64_t)u * pc_nblocks(cout) + n / 32) * 32 + n % 32) * 8 + ci % 8;
}

// Inverse map, as the packing kernel walks it: which element of the OIHW weight tensor W (w_cout, w_cin, 3, 3) lands in
// element j of slot `slot` of a panel; -1 for padding.
//   transposed == 0: the forward panel, a GEMM with cin = w_cin, cout = w_cout, B[k][n] = W[n][ci][ky][kx].
//   transposed == 1: the input-gradient panel, a GEMM with cin = w_cout, cout = w_cin over dY: the same convolution with
//                    flipped, transposed weights, B[k][n] = W[ci][n][2 - ky][2 - kx].
PC_HD int64_t pc_panel_source(int w_cout, int w_cin, int transposed, int64_t slot, int j) {
    const int cin = transposed ? w_cout : w_cin, cout = transposed ? w_cin : w_cout;
    const int nb_total = pc_nblocks(cout), cu = pc_units_per_tap(cin);
    const int n = (int)((slot >> 5) % nb_total) * 32 + (int)(slot & 31);
    const int u = (int)((slot >> 5) / nb_total);
    const int tap = u / cu, ci = (u - tap * cu) * 8 + j;
    if (tap >= 9 || ci >= cin || n >= cout) return -1;
    const int ky = tap / 3, kx = tap - 3 * ky;
    if (!transposed) return (((int64_t)n * w_cin + ci) * 3 + ky) * 3 + kx;
    return (((int64_t)ci * w_cin + n) * 3 + (2 - ky)) * 3 + (2 - kx);
}

// VGG19's widths of conv1_1 .. conv5_1 and the chain's shape: a 2x2 max pool (floor) in FRONT of conv index 2, 4, 8, 12;
// a feature tap behind conv index 0, 2, 4, 8, 12.
PC_HD int pc_vgg19_width(int i) { return i < 2 ? 64 : (i < 4 ? 128 : (i < 8 ? 256 : 512)); }
PC_HD bool pc_pool_before(int i) { return i == 2 || i == 4 || i == 8 || i == 12; }
PC_HD bool pc_is_tap(int i) { return i == 0 || i == 2 || i == 4 || i == 8 || i == 12; }
PC_HD int pc_convs_for_layers(int n_layers) { return n_layers == 1 ? 1 : (n_layers == 2 ? 3 : (n_layers == 3 ? 5 : (n_layers == 4 ? 9 : 13))); }

}  // namespace d3ga
