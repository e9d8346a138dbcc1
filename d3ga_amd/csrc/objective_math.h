// objective_math.h -- the arithmetic and the SUMMATION ORDERS of the training objective (objective.hip): the scale regulariser
// of models/cage_net.py:214, 226 and the assembly of train.py:190-244.  Semantics: DESIGN.md 4.4m (specification of record).
// Compiles for the host as it is (tests/hostcheck/objcheck.cpp runs this very text on the CPU); objective.hip is compiled with
// -ffp-contract=off, so the device evaluates every expression here as g++ does.
//
// Orders, all float32, nothing depends on arrival:
//   an input array of n elements (one "slot" of one frame): lane l of 64 adds the terms of elements l, l + 64, ... in index
//     order (obj_lane_partial); the 64 lane sums meet in a butterfly, partner lane ^ 32, 16, 8, 4, 2, 1 (obj_wave_sum: a + b
//     is commutative, so every lane ends with the same bits);
//   over the frames: f = 0, 1, ... B-1, left to right, then ONE division by B (obj_assemble);
//   the total: color + sil + bg (= 0) + codes + scale + fme + blur + vgg, left to right -- the order of train.py:224-244.
// Every sum is over non-negative terms (squares, |x - 1|, 1 - ssim, energies shifted by 3 BEFORE they are added), so a term's
// relative error is at most (longest lane run + 6 butterfly levels + B frames + the handful of products) * 2^-24:
// n <= D3GA_OBJ_MAX_LEN = 4096 gives runs <= 64, B <= 16, i.e. < 100 * 2^-24 = 6e-6 at the limits and ~20 * 2^-24 at the
// reference's sizes (D = 32, 87 poses, B = 1).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/d3ga.h"

#ifndef D3GA_FHD
#ifdef __HIPCC__
#define D3GA_FHD __host__ __device__ __forceinline__
#else
#define D3GA_FHD static inline
#endif
#endif

namespace d3ga {

constexpr int kObjLanes = 64;
// slots of a frame, the order of d3ga_objective_desc::entry
enum ObjSlot { kObjL1 = 0, kObjSsim, kObjSilL1, kObjScaleEnergy, kObjFmEnergy, kObjEncoding, kObjPoses, kObjBlur, kObjVgg };
// terms, the key order of the reference's `losses` dict (train.py:246-256)
enum ObjTerm { kTermColor = 0, kTermSil, kTermScale, kTermFme, kTermBlur, kTermVgg, kTermBg, kTermCodes, kTermTotal };
constexpr float kObjCodeWeight = 0.001f;      // train.py:195
constexpr float kObjPoseWeight = 0.0075f;     // train.py:198
constexpr float kObjScaleWeight = 175.0f;     // train.py:203
constexpr float kObjFmShift = 3.0f;           // train.py:207

// ---- scale_energy: (1 / n) sum act(scaling + delta)^2 ------------------------------------------------------------------------
// the term of one element and its derivative with respect to x = scaling + delta (both inputs get the same value)
D3GA_FHD float scale_energy_term(int activation, float x) {
    const float a = activation == D3GA_SCALE_ACT_EXP ? expf(x) : x;
    return a * a;
}
D3GA_FHD float scale_energy_dterm(int activation, float x) {
    if (activation != D3GA_SCALE_ACT_EXP) return 2.0f * x;
    const float a = expf(x);                 // d/dx exp(x)^2 = 2 exp(x)^2: an underflowing square gives 0, never 0 * inf
    return 2.0f * (a * a);
}

// ---- the assembly ------------------------------------------------------------------------------------------------------------
D3GA_FHD float obj_elem(int slot, float x) {
    switch (slot) {
    case kObjEncoding:
    case kObjPoses: return x * x;
    case kObjBlur: return fabsf(x - 1.0f);
    case kObjFmEnergy: return x + kObjFmShift;
    default: return x;
    }
}

D3GA_FHD float obj_lane_partial(int slot, const float *p, int n, int lane) {
    float acc = 0.f;
    for (int i = lane; i < n; i += kObjLanes) acc += obj_elem(slot, p[i]);
    return acc;
}

// the butterfly on an array of the 64 lane sums (the device runs it with __shfl_xor); the result is v[0] (= every v[l])
D3GA_FHD float obj_wave_sum(float *v) {
    for (int off = kObjLanes / 2; off >= 1; off >>= 1) {
        float t[kObjLanes];
        for (int l = 0; l < kObjLanes; ++l) t[l] = v[l] + v[l ^ off];
        for (int l = 0; l < kObjLanes; ++l) v[l] = t[l];
    }
    return v[0];
}

D3GA_FHD bool obj_has(const d3ga_objective_desc &d, int slot) { return d.entry[slot].ptr != nullptr; }

// sums: n_frames x D3GA_OBJ_SLOTS, [f][slot] = the wave sum of that entry (the value itself for the 0-d slots; 0 when absent)
D3GA_FHD void obj_assemble(const d3ga_objective_desc &d, const float *sums, float *terms) {
    const int B = d.n_frames;
    const float fB = (float)B;
    float color = 0.f, sil = 0.f, codes = 0.f, scale = 0.f, fme = 0.f, blur = 0.f, vgg = 0.f;
    const float one_minus = 1.0f - d.lambda_dssim;
    for (int f = 0; f < B; ++f) {
        const float *s = sums + f * D3GA_OBJ_SLOTS;
        const d3ga_objective_entry *e = d.entry + f * D3GA_OBJ_SLOTS;
        color += one_minus * s[kObjL1] + d.lambda_dssim * (1.0f - s[kObjSsim]);                    // train.py:193
        sil += s[kObjSilL1];
        float code = kObjCodeWeight * (s[kObjEncoding] / (float)e[kObjEncoding].len);             // :195
        if (e[kObjPoses].ptr) code += kObjPoseWeight * (s[kObjPoses] / (float)e[kObjPoses].len);    // :198
        codes += code;
        scale += kObjScaleWeight * s[kObjScaleEnergy];                                              // :203
        if (e[kObjFmEnergy].ptr) fme += s[kObjFmEnergy] / (float)e[kObjFmEnergy].len;               // :207
        if (e[kObjBlur].ptr) blur += s[kObjBlur] / (float)e[kObjBlur].len;                          // :194
        if (e[kObjVgg].ptr) vgg += s[kObjVgg];
    }
    terms[kTermColor] = color / fB * d.rgb_weight;                                                  // :218
    terms[kTermSil] = sil / fB * d.sil_weight;                                                      // :219
    terms[kTermCodes] = codes / fB;                                                                 // :220
    terms[kTermScale] = scale / (fB * (float)d.entry[kObjScaleEnergy].len);                         // :221
    terms[kTermBg] = 0.f;                                                                           // :222 (never appended to)
    terms[kTermFme] = obj_has(d, kObjFmEnergy) ? fme / fB * d.fme_weight : 0.f;                     // :233
    terms[kTermBlur] = obj_has(d, kObjBlur) ? blur / fB * d.blur_weight : 0.f;                      // :238
    terms[kTermVgg] = obj_has(d, kObjVgg) ? vgg / fB * d.vgg_weight : 0.f;                          // :243
    float total = terms[kTermColor];
    total += terms[kTermSil];
    total += terms[kTermBg];
    total += terms[kTermCodes];
    total += terms[kTermScale];
    if (obj_has(d, kObjFmEnergy)) total += terms[kTermFme];
    if (obj_has(d, kObjBlur)) total += terms[kTermBlur];
    if (obj_has(d, kObjVgg)) total += terms[kTermVgg];
    terms[kTermTotal] = total;
}

// d total / d x of element x of an entry of n elements, for an upstream gradient g
D3GA_FHD float obj_grad(const d3ga_objective_desc &d, int slot, int n, float x, float g) {
    const float fB = (float)d.n_frames, fn = (float)n;
    switch (slot) {
    case kObjL1: return g * ((1.0f - d.lambda_dssim) * d.rgb_weight / fB);
    case kObjSsim: return -(g * (d.lambda_dssim * d.rgb_weight / fB));
    case kObjSilL1: return g * (d.sil_weight / fB);
    case kObjScaleEnergy: return g * (kObjScaleWeight / (fB * fn));
    case kObjFmEnergy: return g * (d.fme_weight / (fB * fn));
    case kObjEncoding: return g * (2.0f * kObjCodeWeight / (fB * fn)) * x;
    case kObjPoses: return g * (2.0f * kObjPoseWeight / (fB * fn)) * x;
    case kObjBlur: {
        const float t = x - 1.0f;                // torch's abs backward: sign(t), 0 at 0; a NaN stays one
        const float sg = t > 0.f ? 1.0f : (t < 0.f ? -1.0f : t);
        return g * (d.blur_weight / (fB * fn)) * sg;
    }
    default: return g * (d.vgg_weight / fB);
    }
}

// The status words (D3GA_OBJ_STATUS_*): count the step; on the FIRST total that is NaN (th.isnan: an infinite one is not)
// remember the step and its nine terms.  Nothing later clears it.
D3GA_FHD void obj_status_update(int32_t *status, const float *terms) {
    const int32_t step = status[D3GA_OBJ_STATUS_STEPS];
    status[D3GA_OBJ_STATUS_STEPS] = step + 1;
    const float total = terms[kTermTotal];
    if (total != total && status[D3GA_OBJ_STATUS_NAN_SEEN] == 0) {
        status[D3GA_OBJ_STATUS_NAN_SEEN] = 1;
        status[D3GA_OBJ_STATUS_FIRST_BAD] = step;
        float *bad = reinterpret_cast<float *>(status + D3GA_OBJ_STATUS_TERMS);
        for (int k = 0; k < D3GA_OBJ_TERMS; ++k) bad[k] = terms[k];
    }
}

}  // namespace d3ga
