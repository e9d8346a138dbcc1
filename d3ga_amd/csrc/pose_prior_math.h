// pose_prior_math.h -- the arithmetic and the SUMMATION ORDERS of the pose prior (pose_prior.hip): the PCA fit over the refined
// poses (test.py:264-274, utils/pca_utils.py:14-24) and the per-frame clamp of test.py:49-56.  Semantics: DESIGN.md 4.4n
// (specification of record).  Compiles for the host as it is (tests/hostcheck/posecheck.cpp runs this very text on the CPU);
// pose_prior.hip is compiled with -ffp-contract=off, so the device evaluates every expression here as g++ does.
//
// Everything is float64; a pose enters as float32 (exact in float64) and leaves through ONE rounding to float32.
// Orders, nothing depends on arrival or on the launch geometry:
//   fit, both passes: the rows of a chunk of kPoseFitChunk rows in ascending order (pp_chunk_sum, pp_chunk_cov), then the
//     chunks in ascending order (pp_chunks_total), then ONE division (by N, by N - 1);
//   projection: z_j = sum over d = 0, 1, ... D-1 of (x_d - mean_d) V_jd (pp_project);
//   reconstruction: (sum over j = 0, 1, ... k-1 of zc_j V_jd) + mean_d (pp_reconstruct).
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

constexpr int kPoseMaxD = D3GA_POSE_MAX_D;
constexpr int kPoseFitChunk = D3GA_POSE_FIT_CHUNK;

D3GA_FHD int pp_chunks(int N) { return (N + kPoseFitChunk - 1) / kPoseFitChunk; }

// ---- fit -----------------------------------------------------------------------------------------------------------------
D3GA_FHD double pp_centre(float x, double mean) { return (double)x - mean; }

// column `col` of rows [r0, r1) of table (., D), in row order
D3GA_FHD double pp_chunk_sum(const float *table, int D, int r0, int r1, int col) {
    double acc = 0.0;
    for (int r = r0; r < r1; ++r) acc += (double)table[(size_t)r * D + col];
    return acc;
}

// one more row of the covariance sum of a pair of columns (the device keeps the centred rows in LDS and calls this per row)
D3GA_FHD double pp_cov_step(double acc, double xi, double xj) { return acc + xi * xj; }

D3GA_FHD double pp_chunk_cov(const float *table, const double *mean, int D, int r0, int r1, int i, int j) {
    double acc = 0.0;
    for (int r = r0; r < r1; ++r)
        acc = pp_cov_step(acc, pp_centre(table[(size_t)r * D + i], mean[i]), pp_centre(table[(size_t)r * D + j], mean[j]));
    return acc;
}

// partial[c * stride] over c = 0 .. chunks-1, in chunk order, divided once
D3GA_FHD double pp_chunks_total(const double *partial, size_t stride, int chunks, double divisor) {
    double s = partial[0];
    for (int c = 1; c < chunks; ++c) s += partial[(size_t)c * stride];
    return s / divisor;
}

// ---- clamp ---------------------------------------------------------------------------------------------------------------
// xc (D): the centred pose; comp_t (D,k): the components, transposed
D3GA_FHD double pp_project(const double *xc, const double *comp_t, int D, int k, int j) {
    double z = 0.0;
    for (int d = 0; d < D; ++d) z += xc[d] * comp_t[(size_t)d * k + j];
    return z;
}

// np.minimum(np.maximum(z, -lim), lim), the reference's order (test.py:53-54); a NaN z fails both tests and stays NaN
D3GA_FHD double pp_clip(double z, double sigma, double std) {
    const double lim = sigma * std;
    double t = z < -lim ? -lim : z;
    t = t > lim ? lim : t;
    return t;
}

// z (k); comp (k,D)
D3GA_FHD float pp_reconstruct(const double *z, const double *comp, const double *mean, int D, int k, int d) {
    double acc = 0.0;
    for (int j = 0; j < k; ++j) acc += z[j] * comp[(size_t)j * D + d];
    return (float)(acc + mean[d]);
}

D3GA_FHD bool pp_stages_valid(int stages) {
    return stages == D3GA_POSE_STAGE_PROJECT || stages == D3GA_POSE_STAGE_RECONSTRUCT ||
           stages == (D3GA_POSE_STAGE_PROJECT | D3GA_POSE_STAGE_CLIP | D3GA_POSE_STAGE_RECONSTRUCT);
}

}  // namespace d3ga
