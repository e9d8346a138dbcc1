// skeleton_math.h -- per-joint math of the momentum-style skeleton kernels (skeleton.hip): Euler angles to quaternion, the
// quaternion product and rotation, the local transform of a joint, the parent -> child chain step, the bind-relative joint
// matrix, and the pullback of each.  Quaternions are float[4] in xyzw order and are used AS GIVEN: nothing is normalised, the
// inverse divides by |q|^2.  A skeleton state is float[8] = translation 3 | quaternion 4 | scale 1.  Also compiled for the host
// (g++, D3GA_HD = static inline) by the arithmetic checks of tests/test_skeleton_host.py, as body_model_math.h is.
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
namespace sk {

constexpr float kLn2 = 0.69314718055994531f;

D3GA_HD void cross3(const float a[3], const float b[3], float o[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// Hamilton product o = a (x) b
D3GA_HD void qmul(const float a[4], const float b[4], float o[4]) {
    o[0] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
    o[1] = -a[0] * b[2] + a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
    o[2] = a[0] * b[1] - a[1] * b[0] + a[2] * b[3] + a[3] * b[2];
    o[3] = -a[0] * b[0] - a[1] * b[1] - a[2] * b[2] + a[3] * b[3];
}

// g = dL/d(a (x) b) -> da, db (overwritten)
D3GA_HD void qmul_bwd(const float a[4], const float b[4], const float g[4], float da[4], float db[4]) {
    da[0] = g[0] * b[3] - g[1] * b[2] + g[2] * b[1] - g[3] * b[0];
    da[1] = g[0] * b[2] + g[1] * b[3] - g[2] * b[0] - g[3] * b[1];
    da[2] = -g[0] * b[1] + g[1] * b[0] + g[2] * b[3] - g[3] * b[2];
    da[3] = g[0] * b[0] + g[1] * b[1] + g[2] * b[2] + g[3] * b[3];
    db[0] = g[0] * a[3] + g[1] * a[2] - g[2] * a[1] - g[3] * a[0];
    db[1] = -g[0] * a[2] + g[1] * a[3] + g[2] * a[0] - g[3] * a[1];
    db[2] = g[0] * a[1] - g[1] * a[0] + g[2] * a[3] - g[3] * a[2];
    db[3] = g[0] * a[0] + g[1] * a[1] + g[2] * a[2] + g[3] * a[3];
}

// o = v + 2 (w (a x v) + a x (a x v)), a = q.xyz, w = q.w: the rotation by q when |q| = 1, and that formula for any q
D3GA_HD void qrot(const float q[4], const float v[3], float o[3]) {
    float av[3], aav[3];
    cross3(q, v, av);
    cross3(q, av, aav);
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = v[i] + 2.f * (av[i] * q[3] + aav[i]);
}

// g = dL/d qrot(q, v) -> dq, dv (overwritten)
D3GA_HD void qrot_bwd(const float q[4], const float v[3], const float g[3], float dq[4], float dv[3]) {
    float av[3], ga[3], gav[3], t0[3], t1[3];
    cross3(q, v, av);
    cross3(g, q, ga);                       // g x a
#pragma unroll
    for (int i = 0; i < 3; ++i) gav[i] = 2.f * (q[3] * g[i] + ga[i]);     // dL/d(a x v)
    cross3(av, g, t0);
    cross3(v, gav, t1);
#pragma unroll
    for (int i = 0; i < 3; ++i) dq[i] = 2.f * t0[i] + t1[i];
    dq[3] = 2.f * (g[0] * av[0] + g[1] * av[1] + g[2] * av[2]);
    cross3(gav, q, t0);
#pragma unroll
    for (int i = 0; i < 3; ++i) dv[i] = g[i] + t0[i];
}

// XYZ Euler angles -> quaternion; the half angles are (-rx/2, ry/2, rz/2)
D3GA_HD void euler_quat(const float r[3], float q[4]) {
    const float h0 = -0.5f * r[0], h1 = 0.5f * r[1], h2 = 0.5f * r[2];
    const float c0 = cosf(h0), c1 = cosf(h1), c2 = cosf(h2), s0 = sinf(h0), s1 = sinf(h1), s2 = sinf(h2);
    q[0] = -s0 * (c1 * c2) - c0 * (s1 * s2);
    q[1] = c0 * (s1 * c2) - s0 * (c1 * s2);
    q[2] = c0 * (c1 * s2) + s0 * (s1 * c2);
    q[3] = c0 * (c1 * c2) - s0 * (s1 * s2);
}

// g = dL/d euler_quat(r) -> dr (overwritten)
D3GA_HD void euler_quat_bwd(const float r[3], const float g[4], float dr[3]) {
    const float h0 = -0.5f * r[0], h1 = 0.5f * r[1], h2 = 0.5f * r[2];
    const float c0 = cosf(h0), c1 = cosf(h1), c2 = cosf(h2), s0 = sinf(h0), s1 = sinf(h1), s2 = sinf(h2);
    const float d0 = g[0] * (-c0 * c1 * c2 + s0 * s1 * s2) + g[1] * (-s0 * s1 * c2 - c0 * c1 * s2) +
                     g[2] * (-s0 * c1 * s2 + c0 * s1 * c2) + g[3] * (-s0 * c1 * c2 - c0 * s1 * s2);
    const float d1 = g[0] * (s0 * s1 * c2 - c0 * c1 * s2) + g[1] * (c0 * c1 * c2 + s0 * s1 * s2) +
                     g[2] * (-c0 * s1 * s2 + s0 * c1 * c2) + g[3] * (-c0 * s1 * c2 - s0 * c1 * s2);
    const float d2 = g[0] * (s0 * c1 * s2 - c0 * s1 * c2) + g[1] * (-c0 * s1 * s2 - s0 * c1 * c2) +
                     g[2] * (c0 * c1 * c2 - s0 * s1 * s2) + g[3] * (-c0 * c1 * s2 - s0 * s1 * c2);
    dr[0] = -0.5f * d0;
    dr[1] = 0.5f * d1;
    dr[2] = 0.5f * d2;
}

// Local transform of a joint from its 7 skeleton parameters p = [t 3 | Euler xyz 3 | log2 scale]:
// translation p.t + offset, rotation prerot (x) q(Euler), scale 2^p[6]
D3GA_HD void local_state(const float p[7], const float offset[3], const float prerot[4], float l[8]) {
    float qe[4];
    euler_quat(p + 3, qe);
    l[0] = p[0] + offset[0]; l[1] = p[1] + offset[1]; l[2] = p[2] + offset[2];
    qmul(prerot, qe, l + 3);
    l[7] = exp2f(p[6]);
}

// g = dL/d(local state); l = that state (its scale is reused) -> dp (overwritten)
D3GA_HD void local_state_bwd(const float p[7], const float prerot[4], const float l[8], const float g[8], float dp[7]) {
    float qe[4], da[4], dqe[4];
    euler_quat(p + 3, qe);
    qmul_bwd(prerot, qe, g + 3, da, dqe);
    euler_quat_bwd(p + 3, dqe, dp + 3);
    dp[0] = g[0]; dp[1] = g[1]; dp[2] = g[2];
    dp[6] = g[7] * l[7] * kLn2;
}

// Child from parent: q = q_p (x) q_l, t = rot(q_p, t_l s_p) + t_p, s = s_p s_l
D3GA_HD void chain_step(const float P[8], const float l[8], float o[8]) {
    const float u[3] = {l[0] * P[7], l[1] * P[7], l[2] * P[7]};
    float r[3];
    qrot(P + 3, u, r);
    o[0] = r[0] + P[0]; o[1] = r[1] + P[1]; o[2] = r[2] + P[2];
    qmul(P + 3, l + 3, o + 3);
    o[7] = P[7] * l[7];
}

// g = dL/d(child state) -> dP, dl (both overwritten)
D3GA_HD void chain_step_bwd(const float P[8], const float l[8], const float g[8], float dP[8], float dl[8]) {
    const float u[3] = {l[0] * P[7], l[1] * P[7], l[2] * P[7]};
    float dq1[4], dq2[4], du[3];
    qmul_bwd(P + 3, l + 3, g + 3, dq1, dl + 3);
    qrot_bwd(P + 3, u, g, dq2, du);
    dP[0] = g[0]; dP[1] = g[1]; dP[2] = g[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) dP[3 + i] = dq1[i] + dq2[i];
    dP[7] = (du[0] * l[0] + du[1] * l[1] + du[2] * l[2]) + g[7] * l[7];
    dl[0] = du[0] * P[7]; dl[1] = du[1] * P[7]; dl[2] = du[2] * P[7];
    dl[7] = g[7] * P[7];
}

// Inverse of a bind state: rotation conj(q) / |q|^2, scale 1 / s, translation rot(q^-1, -t) / s
D3GA_HD void bind_inverse(const float b[8], float o[8]) {
    const float n = 1.f / (b[3] * b[3] + b[4] * b[4] + b[5] * b[5] + b[6] * b[6]);
    o[3] = -b[3] * n; o[4] = -b[4] * n; o[5] = -b[5] * n; o[6] = b[6] * n;
    o[7] = 1.f / b[7];
    const float nt[3] = {-b[0], -b[1], -b[2]};
    float r[3];
    qrot(o + 3, nt, r);
    o[0] = r[0] * o[7]; o[1] = r[1] * o[7]; o[2] = r[2] * o[7];
}

// 3x3 of a quaternion as given (row-major): column c is the unit vector e_c pushed through qrot, so the matrix acts on a
// vector exactly as qrot does -- the rotation matrix when |q| = 1
D3GA_HD void quat_matrix(const float q[4], float R[9]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float e[3] = {c == 0 ? 1.f : 0.f, c == 1 ? 1.f : 0.f, c == 2 ? 1.f : 0.f};
        float col[3];
        qrot(q, e, col);
        R[c] = col[0]; R[3 + c] = col[1]; R[6 + c] = col[2];
    }
}

// G = dL/dR (row-major) -> dq (overwritten): the three columns' qrot pullbacks added up
D3GA_HD void quat_matrix_bwd(const float q[4], const float G[9], float dq[4]) {
    dq[0] = dq[1] = dq[2] = dq[3] = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float e[3] = {c == 0 ? 1.f : 0.f, c == 1 ? 1.f : 0.f, c == 2 ? 1.f : 0.f};
        const float g[3] = {G[c], G[3 + c], G[6 + c]};
        float d[4], de[3];
        qrot_bwd(q, e, g, d, de);
#pragma unroll
        for (int i = 0; i < 4; ++i) dq[i] += d[i];
    }
}

// Joint matrix against the bind state, 3x4 row-major in M[12]: the similarity state (x) bind^-1 -- a chain step with the
// joint's state as the parent and binv = bind_inverse(bind) as the local transform -- written as [R(q) s | t]
D3GA_HD void joint_matrix(const float binv[8], const float s[8], float M[12]) {
    float rel[8], R[9];
    chain_step(s, binv, rel);
    quat_matrix(rel + 3, R);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        M[4 * r] = R[3 * r] * rel[7]; M[4 * r + 1] = R[3 * r + 1] * rel[7]; M[4 * r + 2] = R[3 * r + 2] * rel[7];
        M[4 * r + 3] = rel[r];
    }
}

// G = dL/dM (3x4 row-major) -> ds (overwritten); the bind state is a constant
D3GA_HD void joint_matrix_bwd(const float binv[8], const float s[8], const float G[12], float ds[8]) {
    float rel[8], R[9], GR[9], grel[8], dbinv[8];
    chain_step(s, binv, rel);
    quat_matrix(rel + 3, R);
    grel[7] = 0.f;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            grel[7] += G[4 * r + c] * R[3 * r + c];
            GR[3 * r + c] = G[4 * r + c] * rel[7];
        }
        grel[r] = G[4 * r + 3];
    }
    quat_matrix_bwd(rel + 3, GR, grel + 3);
    chain_step_bwd(s, binv, grel, ds, dbinv);
}

}  // namespace sk
}  // namespace d3ga
