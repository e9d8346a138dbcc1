// CPU build of d3ga_amd/csrc/eval_math.h: the pixel loop of eval.hip with one "thread" per workgroup chunk and the header's
// own per-pixel functions, jet table and PSNR.  Built by tests/test_evaluation_host.py (g++ -ffp-contract=off).
#include <vector>

#include "../../d3ga_amd/csrc/eval_math.h"

using namespace d3ga;

static constexpr JetTable kJet = make_jet_table();

extern "C" {

void hc_eval_jet_table(uint8_t *out) {
    for (int i = 0; i <= kJetBad; ++i)
        for (int c = 0; c < 3; ++c) out[3 * i + c] = kJet.v[i][c];
}

int hc_eval_partials(int H, int W) { return eval_partials((int64_t)H * W); }

// bins of a row of errors
void hc_eval_error_bins(int n, const float *e, int32_t *bins) {
    for (int i = 0; i < n; ++i) bins[i] = eval_error_bin(e[i]);
}

// same arguments as d3ga_eval_frames (include/d3ga.h), host memory; partials in the kernel's layout, each summed pixel by pixel
int hc_eval_frames(int B, int H, int W, int flags, const float *pred, const float *image, const float *alpha, const void *boundary_fg,
                   float *target_out, float *gt_out, float *heat_out, float *partials) {
    const bool composed = (flags & D3GA_EVAL_COMPOSED) != 0, bf32 = (flags & D3GA_EVAL_BOUNDARY_F32) != 0;
    const float bg = (flags & D3GA_EVAL_BG_WHITE) ? 1.f : 0.f;
    const size_t n = (size_t)H * W;
    const int np = eval_partials((int64_t)n);
    const size_t chunk = (size_t)kEvalPass * eval_passes((int64_t)n);
    const int ac = (flags & D3GA_EVAL_ALPHA3) ? 3 : 1;
    for (size_t b = 0; b < (size_t)B; ++b)
        for (int w = 0; w < np; ++w) {
            float acc[3] = {0.f, 0.f, 0.f};
            for (size_t i = w * chunk; i < n && i < (w + 1) * chunk; ++i) {
                const float *p = pred + b * 3 * n + i, *im = image + b * 3 * n + i;
                const float al = composed ? 1.f : alpha[b * ac * n + i];
                const float bd = composed ? 0.f
                                          : (bf32 ? static_cast<const float *>(boundary_fg)[b * n + i]
                                                  : (float)static_cast<const uint8_t *>(boundary_fg)[b * n + i]);
                EvalPixel px;
                eval_pixel(composed, bg, p[0], p[n], p[2 * n], im[0], im[n], im[2 * n], al, bd, &px);
                for (int c = 0; c < 3; ++c) {
                    acc[c] += px.sq[c];
                    if (target_out) target_out[(b * 3 + c) * n + i] = px.target[c];
                    if (heat_out) heat_out[(b * 3 + c) * n + i] = jet_colour(kJet.v[px.bin][c]);
                }
                if (gt_out)
                    for (int c = 0; c < 4; ++c) gt_out[(b * 4 + c) * n + i] = px.gt[c];
            }
            if (partials)
                for (int c = 0; c < 3; ++c) partials[(b * 3 + c) * np + w] = acc[c];
        }
    return 0;
}

// d3ga_eval_ssim + the finishing sum for one frame of three channels: mean ssim_map
double hc_eval_ssim(int H, int W, const float *pred, const float *target) {
    std::vector<float> x(kEvalSsimInputs), y(kEvalSsimInputs), h(5 * kEvalSsimRows);
    double total = 0.0;
    for (int c = 0; c < 3; ++c)
        for (int ty0 = 0; ty0 < H; ty0 += kEvalSsimTile)
            for (int tx0 = 0; tx0 < W; tx0 += kEvalSsimTile)
                total += (double)eval_ssim_tile(x.data(), y.data(), h.data(), pred + (size_t)c * H * W, target + (size_t)c * H * W, H, W, ty0,
                                                tx0, 0, 1, [] {});
    return total / (3.0 * H * W);
}

// d3ga_eval_finish without SSIM: metrics[b] = mean of the per-channel PSNRs, psnr_channels (B,3)
void hc_eval_finish(int B, int H, int W, const float *partials, float *psnr, float *psnr_channels) {
    const int np = eval_partials((int64_t)H * W);
    for (int b = 0; b < B; ++b) {
        double mean = 0.0;
        for (int c = 0; c < 3; ++c) {
            float sum = 0.f;
            for (int i = 0; i < np; ++i) sum += partials[(b * 3 + c) * np + i];
            const double db = eval_psnr_db(sum / (float)((int64_t)H * W));
            psnr_channels[b * 3 + c] = (float)db;
            mean += db;
        }
        psnr[b] = (float)(mean / 3.0);
    }
}
}
