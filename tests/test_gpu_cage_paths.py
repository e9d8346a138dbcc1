"""Every path of the cage operators (d3ga_cage_deform_fwd / _bwd of ABI 112 and d3ga_amd/cage_deform.py) against float64
(oracle.deform through tests/cage_ref.py), at the shapes where a path changes:
  A  the vertex gather of the merge route with long lists (n_segments > 24 V: vertex_gather_kernel over the block partials);
  B  the two C entry points called directly, every output inside a guard band of NaN bit patterns, and every refusal;
  C  lbs_cage_deform against float64 over a pairwise cover of P, K, layout, activations and pose arguments;
  D  degenerate bindings (no Gaussians, one vertex, no vertices, one tetrahedron, unused vertices, int64, strided inputs);
  E  the by-storage plan caches after an in-place edit of an index buffer.
Bars (tests/cage_ref.excess): per Gaussian 1e-3 |ref| + 1e-6 max|ref| + 4x the movement of the float64 result under one float32
rounding of the inputs (four draws); vertex sums with 1e-5 max|ref|; pose gradients through check_pose / pose_floors."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import cage_ref as cr
from d3ga_amd import _lib
from d3ga_amd import cage_deform as cd
from test_gpu_lbs_pose_grad import check_pose, pose_floors

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_NULL, E_SIZE, E_CONFIG = -1, -2, -3            # D3GA_E_* (include/d3ga.h)
PER_GAUSSIAN = ("m", "c", "g_barys", "g_scales", "g_rots")
_FLOAT = ("tmpl", "delta", "A", "w", "Rh", "Th", "tp", "cg_tet", "cg", "barys", "dbary", "scales_log", "scales", "rots", "gm", "gc", "gt")
_INT = ("tetras", "tid", "idx")


def on_device(c):
    return {k: c[k].to(DEV).contiguous() for k in _FLOAT + _INT}


def leaf(t):
    return t.detach().requires_grad_(True)          # (shares the storage and the strides; the operators write no input)


_cases = {}


def case(name, *args, **kw):
    """A case, its device copy and its float64 references (by option), built once per module run and left unchanged."""
    if name not in _cases:
        c = cr.make_case(*args, **kw)
        _cases[name] = (c, on_device(c), {})
    return _cases[name]


def reference(entry, **kw):
    c, _, refs = entry
    key = tuple(sorted(kw.items()))
    if key not in refs:
        refs[key] = cr.reference(c, **kw)
    return refs[key]


def assert_close(got, ref, keys, tag, floor=1e-6, extra_rel=0.0):
    for k in keys:
        e = cr.excess(got[k], ref, k, floor, extra_rel)
        print(f"{tag} {k}: excess {e:.3f}")
        assert e <= 1.0, (tag, k, e)


def run_deform(d, *, exp, per_tet, dbary, merged=True, tetras=None, tid=None, tp=None, inputs=None):
    """cage_deform forward + backward of sum(means gm) + sum(cov6 gc) -> outputs and gradients."""
    x = dict(barys=d["barys"], scales=d["scales_log"] if exp else d["scales"], rots=d["rots"], dbary=d["dbary"],
             tp=d["tp"] if tp is None else tp)
    x.update(inputs or {})
    tpl, b, s, r = leaf(x["tp"]), leaf(x["barys"]), leaf(x["scales"]), leaf(x["rots"])
    db = leaf(x["dbary"]) if dbary else None
    m, c = cd.cage_deform(tpl, d["tetras"] if tetras is None else tetras, d["tid"] if tid is None else tid, b,
                          d["cg_tet"] if per_tet else d["cg"], s, r, delta_barys=db, scale_activation="exp" if exp else None,
                          gradient_per_tet=per_tet)
    cd._merge_policy["enabled"] = merged
    try:
        ((m * d["gm"]).sum() + (c * d["gc"]).sum()).backward()
        torch.cuda.synchronize()
    finally:
        cd._merge_policy["enabled"] = True
    return dict(m=m.detach(), c=c.detach(), g_tp=tpl.grad, g_barys=b.grad, g_scales=s.grad, g_rots=r.grad,
                g_dbary=None if db is None else db.grad)


# ----------------------------------------------------------------------------------------------------------------------------
# A. which vertex gather runs behind the merge route
# ----------------------------------------------------------------------------------------------------------------------------
A_SHAPES = {"V4_T1_P6401": (4, 1, 6401, True, True), "V5_T2_P8000": (5, 2, 8000, True, True),
            "V8_T5_P12545_random_ids": (8, 5, 12545, False, True), "V4_T1_P6144_control": (4, 1, 6144, True, False)}


@pytest.fixture(scope="module", params=list(A_SHAPES))
def gather_case(request):
    V, T, P, sort_ids, long_lists = A_SHAPES[request.param]
    entry = case("A_" + request.param, 300 + list(A_SHAPES).index(request.param), V, T, P, K=1, J=1, sort_ids=sort_ids)
    return request.param, entry, long_lists, {}


@pytest.mark.parametrize("dbary", [False, True], ids=["barys", "delta_barys"])
@pytest.mark.parametrize("per_tet", [False, True], ids=["per_gaussian", "per_tet"])
@pytest.mark.parametrize("exp", [False, True], ids=["scales", "exp"])
def test_gather_path_selection(gather_case, exp, per_tet, dbary):
    """Thousands of Gaussians over a cage of 4 to 8 vertices: more than 24 partials per vertex, so d3ga_cage_deform_bwd hands the
    block partials to vertex_gather_kernel (one wavefront per vertex, indexed through vert_parts) instead of the row kernel; the
    control with exactly 24 per vertex stays on the row kernel.  Merge route against float64, against the corners route
    (2e-5 max + 1e-12 on the vertex gradient, everything else bit-equal) and against itself (bit-equal).
    A vertex here sums up to 12545 float32 terms, in chains of up to 1024 inside a workgroup: the floor of the vertex bar is the
    larger of the project's 1e-5 and 4x the spread of the same float64 terms summed in float32 in two orders on the CPU
    (cage_ref.float32_order_spread; measured 1.1e-6 .. 4.8e-6 on these cases, docs/LOG.md)."""
    name, entry, long_lists, spreads = gather_case
    c, d, _ = entry
    n_segments = cd.merge_plan(d["tetras"], d["tid"], c["V"])["n_segments"]
    assert (n_segments > 24 * c["V"]) == long_lists, (name, n_segments, 24 * c["V"])
    ref = reference(entry, exp=exp, dbary=dbary)
    if (exp, dbary) not in spreads:
        spreads[(exp, dbary)] = cr.float32_order_spread(c, exp=exp, dbary=dbary)
    spread = spreads[(exp, dbary)]
    print(f"{name}: n_segments {n_segments}, float32 order spread {spread:.3e}")
    assert spread < 2.5e-5, "the CPU measurement itself went wrong"
    merge = run_deform(d, exp=exp, per_tet=per_tet, dbary=dbary)
    assert_close(merge, ref, PER_GAUSSIAN, name)
    assert_close(merge, ref, ("g_tp",), name, floor=1e-5, extra_rel=4.0 * spread)
    if dbary:
        assert torch.equal(merge["g_dbary"], merge["g_barys"])
    corners = run_deform(d, exp=exp, per_tet=per_tet, dbary=dbary, merged=False)
    for k in merge:
        if k == "g_tp":
            scale = float(corners[k].abs().max())
            assert float((merge[k] - corners[k]).abs().max()) <= 2e-5 * scale + 1e-12, (name, "merge against corners")
        else:
            assert merge[k] is corners[k] or torch.equal(merge[k], corners[k]), (name, k)
    again = run_deform(d, exp=exp, per_tet=per_tet, dbary=dbary)
    assert torch.equal(again["g_tp"], merge["g_tp"])
    assert float(merge["g_tp"].abs().max()) > 0


# ----------------------------------------------------------------------------------------------------------------------------
# B. d3ga_cage_deform_fwd / d3ga_cage_deform_bwd called directly
# ----------------------------------------------------------------------------------------------------------------------------
B_SIZES = (1, 255, 256, 257, 513)


def direct_case(P):
    """V = 40 of which 37 can be a corner (at least three vertices no Gaussian touches), T = 60, K = 4, J = 7."""
    return case(f"B_P{P}", 500 + P, 40, 60, P, K=4, J=7, vertices_in_tets=37)


def deform_in(c, d, flags, dbary):
    return _lib.CageDeformIn(P=c["P"], V=c["V"], flags=flags, tetpoints=d["tp"].data_ptr(), tetras=d["tetras"].data_ptr(),
                             tetra_id=d["tid"].data_ptr(), barys=d["barys"].data_ptr(),
                             canon_grad=(d["cg_tet"] if flags & 2 else d["cg"]).data_ptr(),
                             scales=(d["scales_log"] if flags & 1 else d["scales"]).data_ptr(), rots=d["rots"].data_ptr(),
                             delta_barys=d["dbary"].data_ptr() if dbary else None)


@pytest.mark.parametrize("flags", [0, 1, 2, 3], ids=["plain", "exp", "per_tet", "exp_per_tet"])
@pytest.mark.parametrize("P", B_SIZES)
def test_direct_forward(P, flags):
    entry = direct_case(P)
    c, d, _ = entry
    dbary = flags in (1, 2)
    out = dict(m=cr.GuardedBuffer("means", (P, 3), DEV), c=cr.GuardedBuffer("cov6", (P, 6), DEV))
    st = deform_in(c, d, flags, dbary)
    status = _lib.lib().d3ga_cage_deform_fwd(ctypes.byref(st), out["m"].ptr(), out["c"].ptr(), _lib.stream_handle())
    torch.cuda.synchronize()
    assert status == 0
    for o in out.values():
        o.check()
    assert_close({k: o.t for k, o in out.items()}, reference(entry, exp=bool(flags & 1), dbary=dbary), ("m", "c"), f"P={P} flags={flags}")
    for bad, want in ((dict(flags=4), E_CONFIG), (dict(P=-1), E_SIZE)):
        fresh = dict(m=cr.GuardedBuffer("means", (P, 3), DEV), c=cr.GuardedBuffer("cov6", (P, 6), DEV))
        for k, v in bad.items():
            setattr(st, k, v)
        assert _lib.lib().d3ga_cage_deform_fwd(ctypes.byref(st), fresh["m"].ptr(), fresh["c"].ptr(), _lib.stream_handle()) == want
        torch.cuda.synchronize()
        for o in fresh.values():
            o.untouched()
        st = deform_in(c, d, flags, dbary)


def combo(outs="bsr", route=None, gtp=False, skin=False, extra=False, rh=False, pose=False, flags=0, dbary=False):
    return dict(outs=outs, route=route, gtp=gtp, skin=skin, extra=extra, rh=rh, pose=pose, flags=flags, dbary=dbary)


B_COMBOS = {"barys_only": combo("b"), "scales_only": combo("s", flags=1), "rots_only": combo("r", flags=2, dbary=True),
            "no_outputs": combo("", flags=3), "corners": combo(route="corners", gtp=True, flags=1, dbary=True),
            "merge": combo(route="merge", gtp=True, flags=2)}
for _n, (_gtp, _extra, _rh) in enumerate(itertools.product((False, True), repeat=3)):
    B_COMBOS["skin" + "_gtp" * _gtp + "_extra" * _extra + "_rh" * _rh] = combo(route="merge", gtp=_gtp, skin=True, extra=_extra, rh=_rh,
                                                                             flags=_n % 4, dbary=bool(_n & 2))
B_COMBOS["skin_pose_extra_rh"] = combo(route="merge", skin=True, extra=True, rh=True, pose=True, flags=1)
B_COMBOS["skin_pose_gtp"] = combo(route="merge", gtp=True, skin=True, pose=True, flags=2, dbary=True)


def direct_backward(entry, cfg, mutate=None):
    """One call of d3ga_cage_deform_bwd with every output in a GuardedBuffer -> (status, {name: GuardedBuffer}).  mutate(S):
    edit the descriptor structs S = dict(inputs, grads, route, skin, pose) (an entry set to None is passed as NULL)."""
    c, d, _ = entry
    P, V = c["P"], c["V"]
    out, keep = {}, []

    def guarded(name, shape, on=True):
        if not on:
            return None
        out[name] = cr.GuardedBuffer(name, shape, DEV)
        return out[name].ptr()
    S = dict(inputs=deform_in(c, d, cfg["flags"], cfg["dbary"]), route=None, skin=None, pose=None)
    S["grads"] = _lib.CageDeformGrads(g_means=d["gm"].data_ptr(), g_cov6=d["gc"].data_ptr(),
                                      g_tetpoints=guarded("g_tp", (V, 3), cfg["gtp"]), g_barys=guarded("g_barys", (P, 4), "b" in cfg["outs"]),
                                      g_scales=guarded("g_scales", (P, 3), "s" in cfg["outs"]), g_rots=guarded("g_rots", (P, 4), "r" in cfg["outs"]))
    if cfg["route"] == "merge":
        plan = cd.merge_plan(d["tetras"], d["tid"], V)
        S["route"] = _lib.CageDeformRoute(kind=_lib.DEFORM_ROUTE_MERGE, n_segments=plan["n_segments"], item_pos=plan["item_pos"].data_ptr(),
                                          seg_ptr=plan["seg_ptr"].data_ptr(), seg_begin=plan["seg_begin"].data_ptr(),
                                          vert_start=plan["vert_start"].data_ptr(), vert_items=plan["vert_parts"].data_ptr(),
                                          records=guarded("records", (plan["n_segments"], 3)))
    elif cfg["route"] == "corners":
        vstart, vitems = cd.vertex_adjacency(d["tetras"], d["tid"], V)
        S["route"] = _lib.CageDeformRoute(kind=_lib.DEFORM_ROUTE_CORNERS, vert_start=vstart.data_ptr(), vert_items=vitems.data_ptr(),
                                          records=guarded("records", (P, 4, 3)))
    if cfg["skin"]:
        S["skin"] = _lib.CageDeformSkin(K=c["K"], joint_mats=d["A"].data_ptr(), skin_idx=d["idx"].data_ptr(), skin_w=d["w"].data_ptr(),
                                        Rh=d["Rh"].data_ptr() if cfg["rh"] else None,
                                        g_tetpoints_extra=d["gt"].data_ptr() if cfg["extra"] else None, g_delta=guarded("g_delta", (V, 3)))
    if cfg["pose"]:
        S["pose"], _, scratch = cd._pose_grad_struct(cd.lbs_pose_plan(d["idx"], c["J"]), V, 1, d["tmpl"], d["delta"], DEV)
        keep.append(scratch)
        S["pose"].g_joint_mats, S["pose"].g_Rh, S["pose"].g_Th = guarded("A", (c["J"], 4, 4)), guarded("Rh", (3, 3)), guarded("Th", (3,))
    if mutate is not None:
        mutate(S)
    ref = lambda x: None if x is None else ctypes.byref(x)
    status = _lib.lib().d3ga_cage_deform_bwd(ref(S["inputs"]), ref(S["grads"]), ref(S["route"]), ref(S["skin"]), ref(S["pose"]),
                                             _lib.stream_handle())
    torch.cuda.synchronize()
    return status, out


@pytest.mark.parametrize("name", list(B_COMBOS))
@pytest.mark.parametrize("P", B_SIZES)
def test_direct_backward(P, name):
    """Every pointer combination the structs allow, at P around the workgroup size: the outputs hold the float64 values, nothing
    is written outside them (64 floats of NaN pattern on either side, bit for bit) and nothing inside is left unwritten; the
    vertices no Gaussian touches get exact zeros."""
    cfg = B_COMBOS[name]
    entry = direct_case(P)
    c, d, _ = entry
    status, out = direct_backward(entry, cfg)
    assert status == 0
    for o in out.values():
        o.check()
    ref = reference(entry, exp=bool(cfg["flags"] & 1), dbary=cfg["dbary"], rh=cfg["rh"], th=cfg["pose"], skin="tail" if cfg["skin"] else None,
                    use="mct" if cfg["extra"] else "mc")
    got = {k: o.t for k, o in out.items()}
    tag = f"P={P} {name}"
    assert_close(got, ref, [k for k in ("g_barys", "g_scales", "g_rots") if k in got], tag)
    assert_close(got, ref, [k for k in ("g_tp", "g_delta") if k in got], tag, floor=1e-5)
    if cfg["pose"]:
        floors = pose_floors(c["tmpl"], c["delta"], c["A"], c["idx"], c["w"], c["Rh"] if cfg["rh"] else None, ref[0]["g_tp"])
        check_pose(dict(A=got["A"], Rh=got["Rh"] if cfg["rh"] else None, Th=got["Th"]), ref[0], floors, tag)
    free = ~cr.touched_vertices(c)
    assert int(free.sum()) >= 3
    if not cfg["extra"]:
        for k in ("g_tp", "g_delta"):
            if k in got:
                assert bool((got[k].cpu()[free] == 0.0).all()), (tag, k, "a vertex without Gaussians")
    if "g_tp" in got:
        assert float(got["g_tp"].abs().max()) > 0


def _set(part, **fields):
    def mutate(S):
        for k, v in fields.items():
            setattr(S[part], k, v)
    return mutate


def _drop(*parts, then=None):
    def mutate(S):
        for p in parts:
            S[p] = None
        if then is not None:
            then(S)
    return mutate


def _shift_item_pos(S):
    S["route"].item_pos += 2


B_REFUSALS = {
    "g_tetpoints_without_route": (_drop("route", "skin", "pose"), E_NULL),
    "route_without_g_tetpoints": (_drop("skin", "pose", then=_set("grads", g_tetpoints=None)), E_NULL),
    "skin_with_corners_route": (_set("route", kind=_lib.DEFORM_ROUTE_CORNERS), E_CONFIG),
    "pose_without_skin": (_drop("skin"), E_CONFIG),
    "unknown_flag": (_set("inputs", flags=4), E_CONFIG),
    "unknown_route_kind": (_set("route", kind=3), E_CONFIG),
    "item_pos_off_by_two_bytes": (_shift_item_pos, E_CONFIG),
    "K_zero": (_set("skin", K=0), E_SIZE),
    "P_negative": (_set("inputs", P=-1), E_SIZE),
    "pose_without_vertices": (_set("inputs", V=0), E_SIZE),
}


@pytest.mark.parametrize("name", list(B_REFUSALS))
def test_direct_backward_refusals(name):
    """Host validation: the status code, and not one float of any output written (nothing is launched)."""
    mutate, want = B_REFUSALS[name]
    cfg = combo(route="merge", gtp=True, skin=True, extra=True, rh=True, pose=True, flags=3, dbary=True)
    status, out = direct_backward(direct_case(257), cfg, mutate)
    assert status == want, (name, status)
    for o in out.values():
        o.untouched()


# ----------------------------------------------------------------------------------------------------------------------------
# C. lbs_cage_deform against float64
# ----------------------------------------------------------------------------------------------------------------------------
ALL = ("tmpl", "delta", "A", "Rh", "Th", "barys", "dbary", "scales", "rots")
# the position of every differentiable input among _LbsCageDeform's arguments
POSITION = dict(tmpl=0, delta=1, A=2, Rh=5, Th=6, barys=9, scales=11, rots=12, dbary=13)


def cell(P, K, per_tet, exp, dbary, rh, th, want=ALL, use="mct", sort_ids=True):
    return dict(P=P, K=K, per_tet=bool(per_tet), exp=bool(exp), dbary=bool(dbary), rh=bool(rh), th=bool(th), want=tuple(want), use=use,
                sort_ids=sort_ids)


# a pairwise cover of P x K x layout x activation x delta_barys x Rh x Th (every pair of values of two factors is in some row)
C_COVER = [(1, 1, 0, 1, 0, 0, 0), (1, 1, 1, 0, 1, 1, 1), (1, 4, 1, 0, 0, 1, 0), (1, 17, 0, 0, 1, 1, 0), (1, 24, 0, 1, 0, 1, 1),
           (255, 1, 0, 0, 0, 0, 1), (255, 4, 1, 1, 0, 0, 1), (255, 17, 1, 0, 1, 1, 1), (255, 24, 0, 0, 1, 1, 0),
           (257, 1, 1, 1, 0, 1, 1), (257, 4, 1, 1, 1, 1, 0), (257, 17, 0, 0, 0, 0, 0), (257, 24, 1, 1, 1, 0, 1),
           (1000, 1, 0, 1, 1, 1, 1), (1000, 4, 0, 0, 0, 1, 1), (1000, 17, 1, 1, 1, 1, 0), (1000, 24, 0, 1, 0, 0, 0)]
for _i, _j in itertools.combinations(range(7), 2):
    _vals = lambda k: sorted({r[k] for r in C_COVER})
    assert {(r[_i], r[_j]) for r in C_COVER} == set(itertools.product(_vals(_i), _vals(_j))), (_i, _j)


def _cell_id(k):
    s = f"P{k['P']}_K{k['K']}_{'per_tet' if k['per_tet'] else 'per_gaussian'}_{'exp' if k['exp'] else 'scales'}"
    return s + "_dbary" * k["dbary"] + "_Rh" * k["rh"] + "_Th" * k["th"]


C_CELLS = {_cell_id(k): k for k in (cell(*r) for r in C_COVER)}
C_CELLS.update({
    "only_delta_P257_K17": cell(257, 17, 1, 1, 1, 1, 1, want=("delta",)),
    "only_joint_mats_P255_K4": cell(255, 4, 0, 1, 0, 1, 0, want=("A",)),
    "only_scales_P1000_K24": cell(1000, 24, 1, 0, 1, 0, 1, want=("scales",)),
    "shuffled_ids_P1000_K4": cell(1000, 4, 1, 1, 1, 1, 1, sort_ids=False),
    "shuffled_ids_P257_K24": cell(257, 24, 0, 0, 0, 1, 1, sort_ids=False),
    "loss_on_tetpoints_only_P255_K17": cell(255, 17, 0, 1, 1, 1, 1, use="t"),
    "loss_on_cov6_only_P1000_K1": cell(1000, 1, 1, 1, 0, 1, 0, use="c"),
})


def run_fused(d, k, *, index=None, inputs=None):
    """lbs_cage_deform forward + backward of the loss terms k['use'] with gradients requested for k['want'] -> (outputs and
    gradients by cage_ref's names, the tuple _LbsCageDeform.backward returned)."""
    x = dict(tmpl=d["tmpl"], delta=d["delta"], A=d["A"], Rh=d["Rh"] if k["rh"] else None, Th=d["Th"] if k["th"] else None,
             barys=d["barys"], scales=d["scales_log"] if k["exp"] else d["scales"], rots=d["rots"], dbary=d["dbary"] if k["dbary"] else None,
             w=d["w"], cg=d["cg_tet"] if k["per_tet"] else d["cg"])
    x.update(inputs or {})
    x.update({n: leaf(x[n]) for n in k["want"] if x[n] is not None})
    ix = dict(idx=d["idx"], tetras=d["tetras"], tid=d["tid"])
    ix.update(index or {})
    m, c, tp = cd.lbs_cage_deform(x["tmpl"], x["delta"], x["A"], ix["idx"], x["w"], ix["tetras"], ix["tid"], x["barys"], x["cg"], x["scales"],
                                  x["rots"], delta_barys=x["dbary"], scale_activation="exp" if k["exp"] else None,
                                  gradient_per_tet=k["per_tet"], Rh=x["Rh"], Th=x["Th"])
    terms = dict(m=lambda: (m * d["gm"]).sum(), c=lambda: (c * d["gc"]).sum(), t=lambda: (tp * d["gt"]).sum())
    loss = sum(terms[u]() for u in k["use"])
    seen, orig = [], cd._LbsCageDeform.backward

    def spy(ctx, *g):
        seen.append(orig(ctx, *g))
        return seen[-1]
    cd._LbsCageDeform.backward = staticmethod(spy)
    try:
        if loss.requires_grad:
            loss.backward()
        torch.cuda.synchronize()
    finally:
        cd._LbsCageDeform.backward = staticmethod(orig)
    g = lambda n: x[n].grad if (n in k["want"] and x[n] is not None) else None
    return dict(m=m.detach(), c=c.detach(), tp=tp.detach(), g_tmpl=g("tmpl"), g_delta=g("delta"), A=g("A"), Rh=g("Rh"), Th=g("Th"),
                g_barys=g("barys"), g_dbary=g("dbary"), g_scales=g("scales"), g_rots=g("rots")), (seen[0] if seen else None)


def check_fused(entry, k, got, returned, tag):
    c = entry[0]
    ref = reference(entry, exp=k["exp"], dbary=k["dbary"], rh=k["rh"], th=k["th"], skin="chain", use=k["use"])
    assert_close(got, ref, ("m", "c", "tp"), tag)
    want = [n for n in k["want"] if not (n == "Rh" and not k["rh"]) and not (n == "Th" and not k["th"]) and not (n == "dbary" and not k["dbary"])]
    assert_close(got, ref, [f"g_{n}" for n in want if n in ("barys", "scales", "rots")], tag)
    if "dbary" in want:
        assert cr.excess(got["g_dbary"], ref, "g_barys") <= 1.0, (tag, "g_dbary")
    assert_close(got, ref, [f"g_{n}" for n in want if n in ("tmpl", "delta")], tag, floor=1e-5)
    if any(n in want for n in ("A", "Rh", "Th")):
        floors = pose_floors(c["tmpl"], c["delta"], c["A"], c["idx"], c["w"], c["Rh"] if k["rh"] else None, ref[0]["g_tp"])
        z = torch.zeros(c["J"], 4, 4)
        check_pose(dict(A=got["A"] if "A" in want else z, Rh=got["Rh"], Th=got["Th"]), dict(ref[0], A=ref[0]["A"] if "A" in want else z.double()),
                   floors, tag)
    assert returned is not None and len(returned) == 15
    for n, pos in POSITION.items():
        assert (returned[pos] is not None) == (n in want), (tag, n, "returned" if returned[pos] is not None else "missing")
    for pos in (3, 4, 7, 8, 10, 14):
        assert returned[pos] is None
    for n in want:
        key = n if n in ("A", "Rh", "Th") else f"g_{n}"
        assert got[key] is not None, (tag, n)


@pytest.mark.parametrize("name", list(C_CELLS))
def test_fused_operator_matches_f64(name):
    """V = 300, J = 9, T = 400: every output and every requested gradient of lbs_cage_deform against the float64 chain
    od.lbs_cage -> od.cage_deform (+ the term on the returned tetpoints), and None for every gradient that was not asked for.
    K = 17 and 24 take a second trip of the row kernel's skinning loop (16 lanes per vertex)."""
    k = C_CELLS[name]
    entry = case(f"C_P{k['P']}_K{k['K']}_{k['sort_ids']}", 700 + k["P"] + k["K"], 300, 400, k["P"], K=k["K"], J=9, sort_ids=k["sort_ids"])
    got, returned = run_fused(entry[1], k)
    check_fused(entry, k, got, returned, name)


# ----------------------------------------------------------------------------------------------------------------------------
# D. degenerate bindings
# ----------------------------------------------------------------------------------------------------------------------------
def test_no_gaussians_cage_deform():
    c, d, _ = case("D_P0", 900, 30, 20, 0, K=4, J=5)
    tp = leaf(d["tp"])
    m, cv = cd.cage_deform(tp, d["tetras"], d["tid"], d["barys"], d["cg"], d["scales"], d["rots"], gradient_per_tet=False)
    assert m.shape == (0, 3) and cv.shape == (0, 6)
    (m.sum() + cv.sum()).backward()
    torch.cuda.synchronize()
    assert tp.grad.shape == (30, 3) and bool((tp.grad == 0.0).all())


@pytest.mark.parametrize("rh,th", [(True, True), (False, False)], ids=["Rh_Th", "no_global_pose"])
def test_no_gaussians_fused_operator(rh, th):
    """P == 0, V > 0: lbs_cage_deform returns lbs_cage's vertices, and a loss on them alone (the FEM term) flows through the
    skinning into delta, template, joint_mats, Rh and Th.  (Refused with D3GA_E_NULL before: the empty plan's tensors have NULL
    pointers.)  The offset gradient is lbs_bwd_kernel's up to the reduction -- the row kernel sums w_k (A_k^T g) over its lanes,
    lbs_bwd_kernel forms (sum_k w_k A_k)^T g -- so it takes the 2e-6 of test_lbs_cage_deform_equals_the_two_operators."""
    entry = case("D_P0", 900, 30, 20, 0, K=4, J=5)
    c, d, _ = entry
    k = cell(0, 4, 0, 1, 1, rh, th, use="t")
    got, returned = run_fused(d, k)
    assert got["m"].shape == (0, 3) and got["c"].shape == (0, 6)
    x = {n: leaf(d[n]) for n in ("tmpl", "delta", "A")}
    Rl, Tl = (leaf(d["Rh"]) if rh else None), (leaf(d["Th"]) if th else None)
    tp = cd.lbs_cage(x["tmpl"], x["delta"], x["A"], d["idx"], d["w"], Rl, Tl)
    assert torch.equal(got["tp"], tp.detach())
    (tp * d["gt"]).sum().backward()
    torch.cuda.synchronize()
    check_fused(entry, k, got, returned, "P == 0")
    scale = float(x["delta"].grad.abs().max())
    assert scale > 0
    for a, b in ((got["g_delta"], x["delta"].grad), (got["g_tmpl"], x["tmpl"].grad)):
        assert float((a - b).abs().max()) <= 2e-6 * scale
    ref = reference(entry, exp=True, dbary=True, rh=rh, th=th, skin="chain", use="t")
    floors = pose_floors(c["tmpl"], c["delta"], c["A"], c["idx"], c["w"], c["Rh"] if rh else None, ref[0]["g_tp"])
    check_pose(dict(A=x["A"].grad, Rh=None if Rl is None else Rl.grad, Th=None if Tl is None else Tl.grad), ref[0], floors, "lbs_cage")
    for n in ("barys", "dbary", "scales", "rots"):
        assert got[f"g_{n}"].shape[0] == 0


@pytest.mark.parametrize("pose", [False, True], ids=["delta_only", "pose"])
def test_one_vertex_one_joint_slot(pose):
    """V == 1, K == 1 through lbs_cage."""
    entry = case("D_V1", 901, 1, 0, 0, K=1, J=3)
    c, d, _ = entry
    delta, A, Rh, Th = leaf(d["delta"]), (leaf(d["A"]) if pose else d["A"]), (leaf(d["Rh"]) if pose else d["Rh"]), (leaf(d["Th"]) if pose else d["Th"])
    out = cd.lbs_cage(d["tmpl"], delta, A, d["idx"], d["w"], Rh, Th)
    (out * d["gt"]).sum().backward()
    torch.cuda.synchronize()
    ref = reference(entry, rh=True, th=True, skin="chain", use="t")
    assert_close(dict(tp=out.detach(), g_delta=delta.grad), ref, ("tp",), "V1")
    assert_close(dict(g_delta=delta.grad), ref, ("g_delta",), "V1", floor=1e-5)
    if pose:
        check_pose(dict(A=A.grad, Rh=Rh.grad, Th=Th.grad), ref[0], pose_floors(c["tmpl"], c["delta"], c["A"], c["idx"], c["w"], c["Rh"], c["gt"]), "V1")
    else:
        assert A.grad is None


@pytest.mark.parametrize("fused", [False, True], ids=["lbs_cage", "lbs_cage_deform"])
def test_no_vertices_with_pose_gradients(fused):
    """V == 0 (and then P == 0): the C ABI takes `pose` with V > 0 only, the operators answer with zeros of the right shapes."""
    c, d, _ = case("D_V0", 902, 0, 0, 0, K=4, J=6)
    delta, A, Rh, Th = leaf(d["delta"]), leaf(d["A"]), leaf(d["Rh"]), leaf(d["Th"])
    if fused:
        m, cv, tp = cd.lbs_cage_deform(d["tmpl"], delta, A, d["idx"], d["w"], d["tetras"], d["tid"], d["barys"], d["cg"], d["scales"], d["rots"],
                                       gradient_per_tet=False, Rh=Rh, Th=Th)
        assert m.shape == (0, 3) and cv.shape == (0, 6)
        loss = m.sum() + cv.sum() + tp.sum()
    else:
        tp = cd.lbs_cage(d["tmpl"], delta, A, d["idx"], d["w"], Rh, Th)
        loss = tp.sum()
    assert tp.shape == (0, 3)
    loss.backward()
    torch.cuda.synchronize()
    for t, shape in ((A, (6, 4, 4)), (Rh, (3, 3)), (Th, (3,)), (delta, (0, 3))):
        assert t.grad is not None and tuple(t.grad.shape) == shape and bool((t.grad == 0.0).all())


D_BINDINGS = {"one_tetrahedron_P600": dict(V=12, T=3, P=600, one_tet=True), "last_workgroup_of_one_P257": dict(V=50, T=80, P=257),
              "half_the_vertices_unused": dict(V=40, T=30, P=700, vertices_in_tets=20)}


@pytest.mark.parametrize("name", list(D_BINDINGS))
@pytest.mark.parametrize("fused", [False, True], ids=["cage_deform", "lbs_cage_deform"])
def test_binding_edges(name, fused):
    """One tetrahedron for 600 Gaussians (segments of 256 items, the last workgroup holds 88), P = 257 (a workgroup of one), half
    the cage outside every tetrahedron (exact zeros there): against float64, both routes of cage_deform."""
    kw = dict(D_BINDINGS[name])
    V, T, P = kw.pop("V"), kw.pop("T"), kw.pop("P")
    entry = case("D_" + name, 910 + list(D_BINDINGS).index(name), V, T, P, K=4, J=5, **kw)
    c, d, _ = entry
    free = ~cr.touched_vertices(c)
    if fused:
        k = cell(P, 4, 1, 1, 1, 1, 1, use="mc")
        got, returned = run_fused(d, k)
        check_fused(entry, k, got, returned, name)
        return
    ref = reference(entry, exp=True, dbary=True)
    for merged in (True, False):
        got = run_deform(d, exp=True, per_tet=True, dbary=True, merged=merged)
        assert_close(got, ref, PER_GAUSSIAN, f"{name} merged={merged}")
        assert_close(got, ref, ("g_tp",), f"{name} merged={merged}", floor=1e-5)
        assert bool((got["g_tp"].cpu()[free] == 0.0).all())
    if name == "half_the_vertices_unused":
        assert int(free.sum()) >= 20


@pytest.mark.parametrize("fused", [False, True], ids=["cage_deform", "lbs_cage_deform"])
def test_int64_indices_equal_int32(fused):
    entry = case("D_int", 920, 60, 90, 700, K=4, J=5)
    d = entry[1]
    i64 = {n: d[n].long() for n in ("tetras", "tid", "idx")}
    if fused:
        k = cell(700, 4, 0, 1, 1, 1, 1)
        a, b = run_fused(d, k)[0], run_fused(d, k, index=i64)[0]
    else:
        a = run_deform(d, exp=True, per_tet=False, dbary=True)
        b = run_deform(d, exp=True, per_tet=False, dbary=True, tetras=i64["tetras"], tid=i64["tid"])
    for n in a:
        assert (a[n] is None and b[n] is None) or torch.equal(a[n], b[n]), n
    assert float(a["g_tp" if not fused else "g_delta"].abs().max()) > 0


@pytest.mark.parametrize("fused", [False, True], ids=["cage_deform", "lbs_cage_deform"])
def test_strided_inputs_equal_contiguous(fused):
    """A [:, :3] slice of a (P,4) tensor for the scales, a column slice for the rotations and barycentrics, a transposed view of
    the stored transpose for the vertices and the offsets: the same bits as their contiguous copies."""
    entry = case("D_int", 920, 60, 90, 700, K=4, J=5)
    d = entry[1]
    wide = lambda t, n: torch.cat([t, torch.full((t.shape[0], n), 7.0, device=DEV)], 1)[:, :t.shape[1]]
    tt = lambda t: t.t().contiguous().t()
    views = dict(scales=wide(d["scales_log"], 1), rots=wide(d["rots"], 3), barys=wide(d["barys"], 4), dbary=tt(d["dbary"]))
    if fused:
        views.update(delta=tt(d["delta"]), tmpl=wide(d["tmpl"], 1), w=tt(d["w"]), A=d["A"].transpose(1, 2).contiguous().transpose(1, 2))
        k = cell(700, 4, 0, 1, 1, 1, 1)
        a, b = run_fused(d, k)[0], run_fused(d, k, inputs=views)[0]
    else:
        views["tp"] = tt(d["tp"])
        a = run_deform(d, exp=True, per_tet=False, dbary=True)
        b = run_deform(d, exp=True, per_tet=False, dbary=True, inputs=views)
    assert not any(v.is_contiguous() for v in views.values())
    for n in a:
        assert (a[n] is None and b[n] is None) or torch.equal(a[n], b[n]), n


# ----------------------------------------------------------------------------------------------------------------------------
# E. plan caches
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
def test_tetra_id_edited_in_place_rebuilds_the_plans(dtype):
    """cage_deform, then `tetra_id.copy_(another assignment)` on the same storage, then cage_deform again: both routes' plans
    (merge_plan, vertex_adjacency) and the cached int32 copy of an int64 buffer follow the edit."""
    old = case("E_old", 930, 50, 70, 600, K=4, J=5)
    new = case("E_new", 931, 50, 70, 600, K=4, J=5)
    d = dict(old[1])
    for n in ("tetras", "tid"):
        d[n] = old[1][n].to(dtype).clone()
    for merged in (True, False):
        first = run_deform(d, exp=False, per_tet=False, dbary=False, merged=merged)
        assert_close(first, reference(old, exp=False, dbary=False), ("g_tp",), "before the edit", floor=1e-5)
        with torch.no_grad():
            d["tid"].copy_(new[1]["tid"])
            d["tetras"].copy_(new[1]["tetras"])
        # the new binding with the old case's floats: its own reference
        c2 = dict(old[0], tid=new[0]["tid"], tetras=new[0]["tetras"], cg=old[0]["cg"])
        ref2 = cr.reference(c2, exp=False, dbary=False)
        second = run_deform(d, exp=False, per_tet=False, dbary=False, merged=merged)
        assert_close(second, ref2, PER_GAUSSIAN, "after the edit")
        assert_close(second, ref2, ("g_tp",), "after the edit", floor=1e-5)
        assert cr.excess(second["g_tp"], reference(old, exp=False, dbary=False), "g_tp", 1e-5) > 1.0      # (the bindings do differ)
        with torch.no_grad():
            d["tid"].copy_(old[1]["tid"])
            d["tetras"].copy_(old[1]["tetras"])


@pytest.mark.parametrize("fused", [False, True], ids=["lbs_cage", "lbs_cage_deform"])
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
def test_skin_idx_edited_in_place_rebuilds_the_pose_plan(dtype, fused):
    old = case("E_old", 930, 50, 70, 600, K=4, J=5)
    new = case("E_new", 931, 50, 70, 600, K=4, J=5)
    d = dict(old[1], idx=old[1]["idx"].to(dtype).clone())
    k = cell(600, 4, 0, 0, 0, 1, 1, use="mct" if fused else "t")

    def run():
        if fused:
            return run_fused(d, k)[0]
        delta, A, Rh, Th = leaf(d["delta"]), leaf(d["A"]), leaf(d["Rh"]), leaf(d["Th"])
        out = cd.lbs_cage(d["tmpl"], delta, A, d["idx"], d["w"], Rh, Th)
        (out * d["gt"]).sum().backward()
        torch.cuda.synchronize()
        return dict(A=A.grad, Rh=Rh.grad, Th=Th.grad, g_delta=delta.grad)
    kw = dict(exp=False, dbary=False, rh=True, th=True, skin="chain", use=k["use"])

    def check(got, c, ref, tag):
        floors = pose_floors(c["tmpl"], c["delta"], c["A"], c["idx"], c["w"], c["Rh"], ref[0]["g_tp"])
        check_pose(got, ref[0], floors, tag)
        assert_close(got, ref, ("g_delta",), tag, floor=1e-5)
    check(run(), old[0], reference(old, **kw), "before the edit")
    with torch.no_grad():
        d["idx"].copy_(new[1]["idx"])
    c2 = dict(old[0], idx=new[0]["idx"])
    ref2 = cr.reference(c2, **kw)
    got = run()
    check(got, c2, ref2, "after the edit")
    assert cr.excess(got["A"], reference(old, **kw), "A") > 1.0


def test_plan_caches_stay_bounded():
    """70 distinct bindings through every by-storage cache: none holds more than limit + 1 entries (host side only)."""
    caches = (cd._i32_cache, cd._adjacency_cache, cd._plan_cache, cd._pose_plan_cache)
    keep = []
    for n in range(70):
        tetras = torch.tensor([[0, 1, 2, 3], [1, 2, 3, 4]], dtype=torch.int64)
        tid = torch.tensor([n % 2, 1, 0], dtype=torch.int64)
        idx = torch.tensor([[n % 3, 1]] * 5, dtype=torch.int64)
        keep.append((tetras, tid, idx))                    # alive: 70 distinct storages
        t32, i32, s32 = cd._i32c(tetras), cd._i32c(tid), cd._i32c(idx)
        keep.append((t32, i32, s32))
        cd.vertex_adjacency(t32, i32, 5)
        assert cd.merge_plan(t32, i32, 5)["n_segments"] == len({int(v) for v in tetras[tid].reshape(-1)})
        assert cd.lbs_pose_plan(s32, 3)["n_entries"] == 10
        for cache in caches:
            assert len(cache.entries) <= cache.limit + 1, (n, len(cache.entries))
    assert max(len(cache.entries) for cache in caches) > 1
