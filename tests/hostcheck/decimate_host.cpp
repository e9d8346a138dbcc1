// CPU build of d3ga_amd/csrc/decimate_math.h: the argument rules and the per-element text of decimate.hip, walked in the kernels'
// order of stages.  Same arguments as the d3ga_decimate_* entry points (include/d3ga.h) without the stream, host memory.
// Built by tests/decimate_ref.py with -ffp-contract=off.
#include "../../d3ga_amd/csrc/decimate_math.h"

using namespace d3ga;

static DcMesh mesh_of(const d3ga_loop_plan *plan, const d3ga_decimate_desc *d) {
    return {plan->V, plan->F, d->x, d->quadrics, d->faces, d->csr_offsets, d->csr_faces};
}

extern "C" {

int64_t hc_decimate_scratch_bytes(int32_t F) { return F <= 0 || 6 * (int64_t)F > INT32_MAX ? (int64_t)D3GA_E_SIZE : dc_scratch_bytes(F); }

int hc_decimate_quadrics(const d3ga_loop_plan *plan, const d3ga_decimate_desc *d) {
    const int st = dc_check_quadrics(plan, d);
    if (st != 0) return st;
    const DcMesh m = mesh_of(plan, d);
    for (int32_t v = 0; v < plan->V; ++v) dc_vertex_quadric(m, v, d->quadrics + 10 * (size_t)v, d->status);
    return 0;
}

int hc_decimate_candidates(const d3ga_loop_plan *plan, const d3ga_decimate_desc *d) {
    const int st = dc_check_candidates(plan, d);
    if (st != 0) return st;
    const DcMesh m = mesh_of(plan, d);
    for (int32_t v = 0; v < plan->V; ++v) { d->owner[v] = kDcNoOwner; d->remap[v] = v; }
    d->counts[1] = 0;
    for (int32_t e = plan->E - 1; e >= 0; --e) {               // any order: here the last edge first
        d->keys[e] = dc_candidate(*plan, m, e, d->placement + 3 * (size_t)e, d->status);
        if (d->keys[e] != kDcBadKey) ++d->counts[1];
    }
    return 0;
}

int hc_decimate_collapse(const d3ga_loop_plan *plan, const d3ga_decimate_desc *d) {
    const int st = dc_check_collapse(plan, d);
    if (st != 0) return st;
    int64_t key;
    int32_t u, w;
    for (int32_t i = d->n_admit - 1; i >= 0; --i) {            // any order of arrival: the minimum is the same
        if (!dc_admitted(*plan, d->sorted_keys, i, &key, &u, &w, d->status)) continue;
        if ((uint64_t)key < d->owner[u]) d->owner[u] = (uint64_t)key;
        if ((uint64_t)key < d->owner[w]) d->owner[w] = (uint64_t)key;
    }
    for (int32_t i = d->n_admit - 1; i >= 0; --i) {
        if (!dc_admitted(*plan, d->sorted_keys, i, &key, &u, &w, d->status)) continue;
        if (!dc_selected(*plan, d->owner, u, w, key, d->status)) continue;
        dc_apply(d->x, d->quadrics, d->remap, u, w, d->placement + 3 * (size_t)dc_key_edge(key));
    }
    return 0;
}

int hc_decimate_faces(const d3ga_loop_plan *plan, const d3ga_decimate_desc *d) {
    const int st = dc_check_faces(plan, d);
    if (st != 0) return st;
    int64_t n = 0;
    for (int32_t f = 0; f < plan->F; ++f) {
        int32_t row[3];
        if (!dc_relabel(plan->V, d->faces, d->remap, f, row, d->status)) continue;
        for (int c = 0; c < 3; ++c) d->faces_out[3 * n + c] = row[c];
        ++n;
    }
    d->counts[0] = n;
    return 0;
}
}
