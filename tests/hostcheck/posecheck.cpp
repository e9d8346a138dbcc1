// CPU build of d3ga_amd/csrc/pose_prior_math.h: the loops of pose_prior.hip with the header's own sums, clip and rounding.
// Built by tests/pose_prior_ref.py (g++ -ffp-contract=off).
#include <vector>

#include "../../d3ga_amd/csrc/pose_prior_math.h"

using namespace d3ga;

extern "C" {

// the four fit kernels: chunk sums in row order, chunks in order, one division; out = mean (D) then covariance (D,D)
int hc_pose_fit(const float *table, int N, int D, double *out) {
    if (N < 2 || D < 1 || D > kPoseMaxD) return D3GA_E_SIZE;
    const int chunks = pp_chunks(N);
    std::vector<double> pmean((size_t)chunks * D), pcov((size_t)chunks * D * D);
    for (int c = 0; c < chunks; ++c) {
        const int r0 = c * kPoseFitChunk, r1 = r0 + kPoseFitChunk < N ? r0 + kPoseFitChunk : N;
        for (int col = 0; col < D; ++col) pmean[(size_t)c * D + col] = pp_chunk_sum(table, D, r0, r1, col);
    }
    for (int col = 0; col < D; ++col) out[col] = pp_chunks_total(pmean.data() + col, (size_t)D, chunks, (double)N);
    for (int c = 0; c < chunks; ++c) {
        const int r0 = c * kPoseFitChunk, r1 = r0 + kPoseFitChunk < N ? r0 + kPoseFitChunk : N;
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j) pcov[(size_t)c * D * D + (size_t)i * D + j] = pp_chunk_cov(table, out, D, r0, r1, i, j);
    }
    for (int e = 0; e < D * D; ++e) out[D + e] = pp_chunks_total(pcov.data() + e, (size_t)D * D, chunks, (double)(N - 1));
    return 0;
}

// pose_clamp_kernel, a pose after the other
int hc_pose_clamp(const float *in, int B, int D, int k, const double *mean, const double *comp, const double *comp_t,
                  const double *std, double sigma, int stages, float *out) {
    if (B < 1 || D < 1 || D > kPoseMaxD || k < 1 || k > kPoseMaxD) return D3GA_E_SIZE;
    if (!pp_stages_valid(stages)) return D3GA_E_CONFIG;
    const bool project = stages & D3GA_POSE_STAGE_PROJECT, reconstruct = stages & D3GA_POSE_STAGE_RECONSTRUCT;
    double xc[kPoseMaxD], z[kPoseMaxD];
    for (int b = 0; b < B; ++b) {
        if (project) {
            for (int d = 0; d < D; ++d) xc[d] = pp_centre(in[(size_t)b * D + d], mean[d]);
            for (int j = 0; j < k; ++j) {
                z[j] = pp_project(xc, comp_t, D, k, j);
                if (stages & D3GA_POSE_STAGE_CLIP) z[j] = pp_clip(z[j], sigma, std[j]);
                if (!reconstruct) out[(size_t)b * k + j] = (float)z[j];
            }
        } else
            for (int j = 0; j < k; ++j) z[j] = (double)in[(size_t)b * k + j];
        if (reconstruct)
            for (int d = 0; d < D; ++d) out[(size_t)b * D + d] = pp_reconstruct(z, comp, mean, D, k, d);
    }
    return 0;
}
}
