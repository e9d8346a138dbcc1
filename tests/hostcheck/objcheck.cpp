// CPU build of d3ga_amd/csrc/objective_math.h: the loops of objective.hip with the header's own per-element functions, lane
// sums, butterfly, assembly, gradients and status update.  Built by tests/objective_ref.py (g++ -ffp-contract=off).
#include "../../d3ga_amd/csrc/objective_math.h"

using namespace d3ga;

extern "C" {

// objective_fwd_kernel: every entry by its 64 lanes and the butterfly, then obj_assemble and the status words
int hc_objective_fwd(const d3ga_objective_desc *d, float *terms, int32_t *status) {
    if (d->n_frames < 1 || d->n_frames > D3GA_OBJ_MAX_FRAMES) return D3GA_E_SIZE;
    float sums[D3GA_OBJ_MAX_FRAMES * D3GA_OBJ_SLOTS];
    for (int it = 0; it < d->n_frames * D3GA_OBJ_SLOTS; ++it) {
        const d3ga_objective_entry &e = d->entry[it];
        float v[kObjLanes];
        for (int l = 0; l < kObjLanes; ++l) v[l] = e.ptr ? obj_lane_partial(it % D3GA_OBJ_SLOTS, e.ptr, e.len, l) : 0.f;
        sums[it] = obj_wave_sum(v);
    }
    obj_assemble(*d, sums, terms);
    obj_status_update(status, terms);
    return 0;
}

// objective_bwd_kernel
int hc_objective_bwd(const d3ga_objective_desc *d, float g, float *grads) {
    for (int it = 0; it < d->n_frames * D3GA_OBJ_SLOTS; ++it) {
        const d3ga_objective_entry &e = d->entry[it];
        if (!e.ptr || e.goff < 0) continue;
        for (int i = 0; i < e.len; ++i) grads[e.goff + i] = obj_grad(*d, it % D3GA_OBJ_SLOTS, e.len, e.ptr[i], g);
    }
    return 0;
}

// scale_energy's terms, summed in float64 (the kernel's two-stage order is a GPU matter), and its gradient
float hc_scale_energy(int64_t n, const float *scaling, const float *delta, int activation, float g, float *grad) {
    double s = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        const float x = delta ? scaling[i] + delta[i] : scaling[i];
        s += (double)scale_energy_term(activation, x);
        if (grad) grad[i] = g / (float)n * scale_energy_dterm(activation, x);
    }
    return (float)(s / (double)n);
}
}
