"""Float64 restatement of the barycentric attribute interpolation (d3ga_amd/bary_interp.py, include/d3ga.h D2b) and the error
bars its tests hold the kernels to: index, einsum, autograd -- the reference's own formulation (models/cage_net.py:236-241,270;
models/mesh_net.py:193,226) in double precision, plus the sums over absolute values the bars are multiples of.

Bars (derived, not measured; u = 2^-24, exact quantities in float64):
    out      |a - b| <= (K + 2) u S_out      S_out   = sum_k |w_k| |a_k|
    g_barys  |a - b| <= (C + 1) u S_barys    S_barys = sum_c |a_c| |g_c|
    g_attr   |a - b| <= (L_v + 3) u S_attr   S_attr  = sum over the items of v of |w| |g|,  L_v = the length of v's list
the standard bound of a float32 sum in any order plus the rounding of w = barys + delta_barys.  Against a float32 result of the
reference twice the bar, because its sum obeys the same bound.  No outliers, no element left out."""
import numpy as np
import torch

U = 2.0 ** -24


def final_rows(rows=None, cells=None, cell_id=None, vertex_map=None):
    """The (P,K) int64 table a binding stands for, by plain indexing."""
    r = rows.long() if rows is not None else cells.long()[cell_id.long()]
    return r if vertex_map is None else vertex_map.long()[r]


def brute_force_lists(rows, n_rows):
    """Per row v the items K i + k that read it, ascending -- by a Python loop over the table."""
    P, K = rows.shape
    lists = [[] for _ in range(n_rows)]
    for i in range(P):
        for k in range(K):
            lists[int(rows[i, k])].append(K * i + k)
    return lists


def _einsum(attr, rows, w):
    return torch.einsum("ikj,ik->ij", attr[rows], w)


def interp_ref(attr, rows, barys, delta_barys=None, g_out=None):
    """Everything in float64 from the given (float32) inputs.  attr (V,C) | (V,), rows (P,K) int, barys / delta_barys (P,K),
    g_out (P,C) | None -> dict(out, S_out, and with g_out: g_attr, g_barys, S_attr, S_barys, L (V,) list lengths)."""
    attr = attr.detach().double().cpu()
    attr = (attr[:, None] if attr.dim() == 1 else attr).clone().requires_grad_(True)
    rows = rows.long().cpu()
    w = barys.detach().double().cpu()
    if delta_barys is not None:
        w = w + delta_barys.detach().double().cpu()
    w = w.clone().requires_grad_(True)
    out = _einsum(attr, rows, w)
    a_abs, w_abs = attr.detach().abs().requires_grad_(True), w.detach().abs().requires_grad_(True)
    s_out = _einsum(a_abs, rows, w_abs)
    res = dict(out=out.detach(), S_out=s_out.detach())
    if g_out is not None:
        g = g_out.detach().double().cpu().reshape(out.shape)
        if out.numel():
            res["g_attr"], res["g_barys"] = torch.autograd.grad(out, [attr, w], g)
            res["S_attr"], res["S_barys"] = torch.autograd.grad(s_out, [a_abs, w_abs], g.abs())
        else:
            res["g_attr"], res["S_attr"] = torch.zeros_like(attr), torch.zeros_like(attr)
            res["g_barys"], res["S_barys"] = torch.zeros_like(w), torch.zeros_like(w)
        res["L"] = torch.bincount(rows.reshape(-1), minlength=attr.shape[0]).double()
    return res


def bars(ref, K, C):
    """The three bars as tensors shaped like the outputs (g_* only when the reference carries gradients)."""
    b = dict(out=(K + 2) * U * ref["S_out"])
    if "g_attr" in ref:
        b["g_barys"] = (C + 1) * U * ref["S_barys"]
        b["g_attr"] = (ref["L"][:, None] + 3) * U * ref["S_attr"]
    return b


def assert_within(name, got, want, bar, factor=1.0):
    """Every element of `got` within factor x bar of `want`; prints the worst ratio before asserting."""
    got, want = torch.as_tensor(got).detach().double().cpu().reshape(bar.shape), want.reshape(bar.shape)
    assert torch.isfinite(got).all(), f"{name}: non-finite values (an element was not written?)"
    err = (got - want).abs()
    allow = factor * bar
    worst = float((err / allow.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"[bary] {name}: max |a - b| {float(err.max()) if err.numel() else 0.0:.3e}, worst share of the bar {worst:.3f}")
    bad = err > allow
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.numel()} elements beyond the bar (worst x{worst:.2f})"


def golden_cases(gd):
    """The three cases of interp_cases.npz as dicts of CPU tensors: attr, binding arguments, barys, delta, the reference's
    float32 output, its upstream gradient and its float32 gradients (None where the reference formed none)."""
    t = lambda k: torch.from_numpy(np.asarray(gd[k]))
    return {
        "shadow": dict(attr=t("c_pred_ao"), bind=dict(cells=t("c_tetras"), cell_id=t("c_tetra_id"), vertex_map=t("c_vertex_map")),
                       barys=t("c_barys"), delta=t("c_delta_bary"), out=t("c_shadow"), up=t("c_up_shadow"),
                       g_attr=t("c_grad_pred_ao"), g_barys=t("c_grad_delta_bary")),
        "canonical": dict(attr=t("c_canon_points"), bind=dict(cells=t("c_tetras"), cell_id=t("c_tetra_id")), barys=t("c_barys"),
                          delta=None, out=t("c_canonical_means3D"), up=None, g_attr=None, g_barys=None),
        "mesh": dict(attr=t("m_points"), bind=dict(rows=t("m_face_ids")), barys=t("m_barys"), delta=t("m_delta_bary"),
                     out=t("m_means3D"), up=t("m_up_means"), g_attr=t("m_grad_points"), g_barys=t("m_grad_delta_bary")),
        "mesh_canonical": dict(attr=t("m_points"), bind=dict(rows=t("m_face_ids")), barys=t("m_barys"), delta=None,
                               out=t("m_canonical_means3D"), up=None, g_attr=None, g_barys=None),
    }
