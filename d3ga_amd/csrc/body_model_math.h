// body_model_math.h -- per-element math of the SMPL(-X) body model kernels (body_model.hip): Rodrigues forward and
// backward, 3x3 products and the rigid 4x4 compose.  Row-major 3x3 matrices in float[9].  Also compiled for the host by the
// arithmetic self-check in tests/hostcheck (g++, D3GA_HD = static inline), as d3ga_math.h is.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#else
#include <cmath>
#endif

#ifndef D3GA_HD
#ifdef __HIPCC__
#define D3GA_HD __host__ __device__ __forceinline__
#else
#define D3GA_HD static inline
#endif
#endif

namespace d3ga {
namespace bm {

constexpr float kRodEps = 1e-8f;   // t = |r + eps| (d3ga_amd.cage_deform.batch_rodrigues): keeps the zero rotation finite

// R = I + sin(t) K + (1 - cos t) K^2, t = |r + eps|, K = [r / t]x.  1 - cos t is formed as 2 sin^2(t/2) (no cancellation).
D3GA_HD void rodrigues(const float r[3], float R[9]) {
    const float ex = r[0] + kRodEps, ey = r[1] + kRodEps, ez = r[2] + kRodEps;
    const float t = sqrtf(ex * ex + ey * ey + ez * ez);
    const float kx = r[0] / t, ky = r[1] / t, kz = r[2] / t;
    const float s = sinf(t), h = sinf(0.5f * t), omc = 2.f * h * h;
    // K^2 = k k^T - |k|^2 I
    const float kk = kx * kx + ky * ky + kz * kz;
    R[0] = 1.f + omc * (kx * kx - kk); R[1] = -s * kz + omc * kx * ky;      R[2] = s * ky + omc * kx * kz;
    R[3] = s * kz + omc * ky * kx;      R[4] = 1.f + omc * (ky * ky - kk);  R[5] = -s * kx + omc * ky * kz;
    R[6] = -s * ky + omc * kz * kx;     R[7] = s * kx + omc * kz * ky;      R[8] = 1.f + omc * (kz * kz - kk);
}

// dL/dr from G = dL/dR of rodrigues(r)
D3GA_HD void rodrigues_bwd(const float r[3], const float G[9], float dr[3]) {
    const float ex = r[0] + kRodEps, ey = r[1] + kRodEps, ez = r[2] + kRodEps;
    const float t = sqrtf(ex * ex + ey * ey + ez * ez);
    const float k[3] = {r[0] / t, r[1] / t, r[2] / t};
    const float s = sinf(t), c = cosf(t), h = sinf(0.5f * t), omc = 2.f * h * h;
    const float K[9] = {0.f, -k[2], k[1], k[2], 0.f, -k[0], -k[1], k[0], 0.f};
    float KK[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) KK[3 * i + j] = K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j] + K[3 * i + 2] * K[6 + j];
    float gK = 0.f, gKK = 0.f;
#pragma unroll
    for (int i = 0; i < 9; ++i) { gK += G[i] * K[i]; gKK += G[i] * KK[i]; }
    const float da = c * gK + s * gKK;              // d sin / dt = cos, d (1 - cos) / dt = sin
    // dL/dK = s G + (1 - cos)(G K^T + K^T G)
    float dK[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float gkt = 0.f, ktg = 0.f;
#pragma unroll
            for (int m = 0; m < 3; ++m) { gkt += G[3 * i + m] * K[3 * j + m]; ktg += K[3 * m + i] * G[3 * m + j]; }
            dK[3 * i + j] = s * G[3 * i + j] + omc * (gkt + ktg);
        }
    const float dk[3] = {dK[7] - dK[5], dK[2] - dK[6], dK[3] - dK[1]};
    // k = r / t, t = |r + eps|
    const float kdk = (dk[0] * r[0] + dk[1] * r[1] + dk[2] * r[2]) / (t * t);
    const float dt = da - kdk;
    dr[0] = dk[0] / t + dt * ex / t;
    dr[1] = dk[1] / t + dt * ey / t;
    dr[2] = dk[2] / t + dt * ez / t;
}

D3GA_HD void mm3(const float a[9], const float b[9], float o[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) o[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

D3GA_HD void mv3(const float a[9], const float v[3], float o[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = a[3 * i] * v[0] + a[3 * i + 1] * v[1] + a[3 * i + 2] * v[2];
}

D3GA_HD void mtv3(const float a[9], const float v[3], float o[3]) {    // a^T v
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = a[i] * v[0] + a[3 + i] * v[1] + a[6 + i] * v[2];
}

// rigid compose [Rp | tp] . [R | t] -> [Rp R | Rp t + tp]
D3GA_HD void compose(const float Rp[9], const float tp[3], const float R[9], const float t[3], float Ro[9], float to[3]) {
    mm3(Rp, R, Ro);
    mv3(Rp, t, to);
    to[0] += tp[0]; to[1] += tp[1]; to[2] += tp[2];
}

}  // namespace bm
}  // namespace d3ga
