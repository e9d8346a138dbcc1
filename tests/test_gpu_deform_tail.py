"""The cage deformation's per-Gaussian backward as the tail of the rasterizer's per-Gaussian backward
(d3ga_raster_preprocess_bwd_deform, preprocess_bwd_kernel<false, true>; cage_deform.set_render_fusion).

The comparison side is always the two-kernel path of the same build -- d3ga_raster_preprocess_bwd, then d3ga_cage_deform_bwd --
which is what runs with set_render_fusion(False).

Native (one compositing backward, both sides on identical copies of its accumulator): dL/dSH, dL/dopacity, dL/dmean2D and, when
requested, dL/dmean and dL/dcov must be bit-identical.  g_barys, g_scales, g_rots, the route's records and the vertex / skinning /
pose gradients are expected bit-identical too (both sides inline the same preprocess_bwd_one arithmetic and deform_bwd); should
the compiler contract the two inlined copies differently, the bar is 4 x side A's own distance to the float64 oracle
(oracle/deform.py on A's dL/dmean, dL/dcov) on these inputs -- never a number taken from the fused side.  Measured: the register
variant of the kernel does differ in the last bit of dL/dmean (docs/LOG.md, "Deform backward as the tail ..."); A's distance to
the oracle is 4.0e-7 .. 1.1e-6 at P = 1 .. 577, the two sides differ by less than that.  With the two arrays requested the kernel
variant that writes them is bit-identical to side A in every output.

Autograd (whole step): the compositing backward's float atomics arrive in another order every run, so the unfused side's own
spread over five runs is measured and 8 x that is allowed, capped at 2e-2 of the largest element of the gradient."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from util import scene_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
ORACLE_MULTIPLE = 4.0


@functools.lru_cache(maxsize=None)
def _scene():
    return scene_inputs("T1", scale_mult=3.0)


def _d(t):
    return None if t is None else t.to(DEV).contiguous()


def _leaf(t):
    return t.to(DEV).clone().contiguous().requires_grad_(True)


def _cull_mask_spread(P):
    """One Gaussian per wavefront (as _spread of the binning test): index i -> 64 i, the other 63 of its wavefront culled copies."""
    idx = torch.arange(64 * P) // 64
    keep = torch.zeros(64 * P, dtype=torch.bool)
    keep[::64] = True
    return idx, ~keep


def _deform_node(idx, *, kind="cage", per_tet=False, delta_barys=False, exp=False, want_tetpoints=True, pose=False, seed=0):
    """The deform forward on the Gaussians `idx` of T1 -> (means, cov6, leaves by name).  kind: "cage" (cage_deform on leaf or
    constant tetpoints) | "lbs" (lbs_cage_deform; pose: joint_mats wants a gradient)."""
    from d3ga_amd import cage_deform as cd
    inp = _scene()
    sc = inp["scene"]
    gen = torch.Generator().manual_seed(seed)
    tetras, tid = _d(sc["tetras"]), _d(sc["tetra_id"][idx])
    barys = _leaf(sc["barys"][idx])
    cg = _d(cd.canonical_gradient_per_tet(sc["canon_points"], sc["tetras"]) if per_tet else inp["canon_grad"][idx])
    scales = _leaf(sc["scaling"][idx] + float(np.log(3.0)) if exp else inp["scales"][idx])
    rots = _leaf(sc["rotation"][idx])
    db = _leaf(0.01 * torch.randn(len(idx), 4, generator=gen)) if delta_barys else None
    kw = dict(delta_barys=db, scale_activation="exp" if exp else None, gradient_per_tet=per_tet)
    leaves = dict(barys=barys, scales=scales, rots=rots)
    if db is not None:
        leaves["delta_barys"] = db
    if kind == "cage":
        tp = _leaf(inp["tetpoints"]) if want_tetpoints else _d(inp["tetpoints"])
        if want_tetpoints:
            leaves["tetpoints"] = tp
        means, cov6 = cd.cage_deform(tp, tetras, tid, barys, cg, scales, rots, **kw)
    else:
        delta = _leaf(sc["delta_node"])
        A = _leaf(sc["joint_mats"]) if pose else _d(sc["joint_mats"])
        leaves["delta"] = delta
        if pose:
            leaves["joint_mats"] = A
        means, cov6, _ = cd.lbs_cage_deform(_d(sc["canon_points"]), delta, A, _d(sc["skin_idx"]), _d(sc["skin_w"]), tetras, tid, barys, cg,
                                            scales, rots, **kw)
    return means, cov6, leaves


def _native_ab(idx, cull=None, want_geo=False, **node_kw):
    """One forward and one compositing backward on the Gaussians `idx` (those of `cull` moved behind the camera for the
    rasterizer), then side A (two kernels) and side B (fused kernel + tails) on copies of the accumulator.
    -> (A, B): dicts of every output, and the float64-oracle distance of A's per-Gaussian deform gradients."""
    from d3ga_amd import _lib
    from d3ga_amd import cage_deform as cd
    from d3ga_amd import rasterizer as R
    from d3ga_amd._lib import check, dptr, stream_handle
    inp = _scene()
    P = len(idx)
    cd.set_render_fusion(False)                        # the forward below must not claim the node: both sides are driven by hand
    try:
        means, cov6, _ = _deform_node(idx, **node_kw)
    finally:
        cd.set_render_fusion(True)
    node = means.grad_fn
    m_r = means.detach().clone()
    if cull is not None:
        m_r[cull.to(DEV), 2] -= 100.0
    m_r.requires_grad_(True)
    settings = R.GaussianRasterizationSettings(
        image_height=inp["H"], image_width=inp["W"], tanfovx=inp["cam"]["tanfovx"], tanfovy=inp["cam"]["tanfovy"],
        bg=torch.tensor([0.2, 0.4, 0.6], device=DEV), scale_modifier=1.0, viewmatrix=_d(inp["view"]).float(), projmatrix=_d(inp["proj"]).float(),
        sh_degree=3, campos=_d(inp["campos"]).float(), prefiltered=False, debug=False, antialiasing=False)
    target = torch.rand(3, inp["H"], inp["W"], generator=torch.Generator().manual_seed(5)).to(DEV)
    out = R.rasterize_gaussians_l1(m_r, None, _d(inp["shs"][idx]), None, _d(inp["opacities"][idx]), None, None, cov6.detach(), settings, target,
                                   want_invdepth=False)
    ctx = out[3].grad_fn
    (m3, sh, _s, _r, c6, view, proj, campos, bg, geom, binning, img, _c2, _b2, image, l1_t, l1_cell) = ctx.saved_tensors
    prm, cap = ctx.prm, ctx.cap
    assert not prm.acc_self_clearing
    L, st, pp = _lib.lib(), stream_handle(), ctypes.byref(ctx.prm)
    new = lambda *s: torch.empty(s, dtype=torch.float32, device=DEV)
    acc = torch.zeros(P, _lib.ACC_STRIDE, device=DEV)
    check(L.d3ga_raster_composite_bwd_l1(pp, dptr(bg), dptr(geom), dptr(binning), cap, dptr(img), dptr(image), dptr(l1_t), dptr(l1_cell),
                                         dptr(torch.ones(1, device=DEV)), None, dptr(acc), st), "d3ga_raster_composite_bwd_l1")
    inputs, flags, wants, lbs, want_v = cd._node_state(node)
    skin = pose = None
    if lbs:
        skin, pose = cd._lbs_saved(node, node.saved_tensors[8:])
        skin = dict(skin, g_extra=None)
    # side A: the two kernels
    a_acc = acc.clone()
    A = dict(gm=new(P, 3), gcov=new(P, 6), gm2d=new(P, 3), gop=new(P, 1), gsh=new(P, 16, 3))
    check(L.d3ga_raster_preprocess_bwd(pp, dptr(m3), dptr(sh), None, None, dptr(c6), dptr(view), dptr(proj), dptr(campos), dptr(geom),
                                       dptr(a_acc), dptr(A["gm"]), dptr(A["gm2d"]), dptr(A["gop"]), dptr(A["gsh"]), None, dptr(A["gcov"]),
                                       None, None, st), "d3ga_raster_preprocess_bwd")
    A.update(gb=new(P, 4) if wants["want_barys"] else None, gs=new(P, 3) if wants["want_scales"] else None,
             gr=new(P, 4) if wants["want_rotations"] else None)
    A["gv"], A["pose"], A["records"] = cd._deform_call("d3ga_cage_deform_bwd", inputs, flags, A["gm"], A["gcov"], A["gb"], A["gs"], A["gr"],
                                                       want_tetpoints=bool(want_v) and not lbs, skin=skin, pose=pose)
    # side B: the fused kernel, then the tails alone
    b_acc = acc.clone()
    B = dict(gm=new(P, 3) if want_geo else None, gcov=new(P, 6) if want_geo else None, gm2d=new(P, 3), gop=new(P, 1), gsh=new(P, 16, 3))
    dst, dgr, route, dep = cd.fused_tail_structs(node)
    ref = lambda x: None if x is None else ctypes.byref(x)
    check(L.d3ga_raster_preprocess_bwd_deform(pp, dptr(m3), dptr(sh), None, None, dptr(c6), dptr(view), dptr(proj), dptr(campos), dptr(geom),
                                              dptr(b_acc), dptr(B["gm"]), dptr(B["gm2d"]), dptr(B["gop"]), dptr(B["gsh"]), None, dptr(B["gcov"]),
                                              None, None, ref(dst), ref(dgr), ref(route), st), "d3ga_raster_preprocess_bwd_deform")
    B.update(gb=dep["barys"], gs=dep["scales"], gr=dep["rotations"], records=dep["records"], gv=None, pose=None)
    if dep["records"] is not None:
        B["gv"], B["pose"], _ = cd._deform_call("d3ga_cage_deform_bwd_tail", inputs, flags, None, None, None, None, None,
                                                want_tetpoints=bool(want_v) and not lbs, skin=skin, pose=pose,
                                                route_records=(dep["records"], dep["merged"]))
    torch.cuda.synchronize()
    assert torch.equal(a_acc, b_acc)
    return A, B, inputs, flags


def _oracle_distance(A, inputs, flags):
    """max-norm relative distance of side A's (g_barys, g_scales, g_rots) to the float64 oracle on A's own dL/dmean, dL/dcov"""
    from oracle import deform as od
    cpu = lambda t: None if t is None else t.detach().cpu().double()
    tp, barys, sc, rot = (cpu(inputs[k]).requires_grad_(k != "tetpoints") for k in ("tetpoints", "barys", "scales", "rotations"))
    b = barys if inputs["delta_barys"] is None else barys + cpu(inputs["delta_barys"])
    cg = cpu(inputs["canon_grad"])
    if flags & 2:
        cg = cg[inputs["tetra_id"].cpu().long()]
    m, c = od.cage_deform(tp, inputs["tetras"].cpu(), inputs["tetra_id"].cpu(), b, cg, torch.exp(sc) if flags & 1 else sc, rot)
    ((m * cpu(A["gm"])).sum() + (c * cpu(A["gcov"])).sum()).backward()
    worst = 0.0
    for mine, ref in ((A["gb"], barys.grad), (A["gs"], sc.grad), (A["gr"], rot.grad)):
        if mine is not None:
            worst = max(worst, float((cpu(mine) - ref).abs().max() / (ref.abs().max() + 1e-30)))
    return worst


def _assert_sides(A, B, inputs, flags, what, want_geo=False):
    for k in ("gsh", "gop", "gm2d") + (("gm", "gcov") if want_geo else ()):
        assert torch.equal(A[k], B[k]), (what, k, float((A[k] - B[k]).abs().max()))
    pairs = [(k, A[k], B[k]) for k in ("gb", "gs", "gr", "records", "gv")]
    if A["pose"] is not None:
        pairs += [(f"pose{j}", a, b) for j, (a, b) in enumerate(zip(A["pose"], B["pose"]))]
    differ = [(k, a, b) for k, a, b in pairs if (a is None) != (b is None) or (a is not None and not torch.equal(a, b))]
    if not differ:
        return
    dist = _oracle_distance(A, inputs, flags)
    print(f"{what}: not bit-identical in {[k for k, _, _ in differ]}; side A's distance to the float64 oracle {dist:.3e}")
    for k, a, b in differ:
        assert a is not None and b is not None, (what, k)
        err = float((a - b).abs().max() / (a.abs().max() + 1e-30))
        assert err <= ORACLE_MULTIPLE * dist, (what, k, err, dist)


# the decimations of tests/test_gpu_binning_reserve.py: a partial, a nearly full, a full wavefront and one Gaussian into the second;
# the same around a block; a last wavefront of one Gaussian in a third block
@pytest.mark.parametrize("P", [1, 63, 64, 65, 255, 257, 577])
def test_native_gaussian_counts(P):
    idx = torch.arange(P) * 5
    A, B, inputs, flags = _native_ab(idx, kind="lbs", delta_barys=True, exp=True)
    assert float(A["gsh"].abs().max()) > 0 and float(A["gb"].abs().max()) > 0
    _assert_sides(A, B, inputs, flags, f"P={P}")


def test_native_geometry_gradients_on_request():
    idx = torch.arange(577) * 5
    A, B, inputs, flags = _native_ab(idx, want_geo=True, kind="lbs", delta_barys=True, exp=True)
    assert float(A["gm"].abs().max()) > 0 and float(A["gcov"].abs().max()) > 0
    _assert_sides(A, B, inputs, flags, "geometry gradients", want_geo=True)


BRANCHES = {
    "per_gaussian_plain": dict(kind="cage"),
    "per_tet": dict(kind="cage", per_tet=True),
    "delta_barys": dict(kind="cage", delta_barys=True),
    "exp": dict(kind="cage", exp=True),
    "corners": dict(kind="cage", merge=False),
    "no_vertex_gradient": dict(kind="cage", want_tetpoints=False),
    "lbs": dict(kind="lbs", per_tet=True, delta_barys=True, exp=True),
    "lbs_pose": dict(kind="lbs", pose=True),
}


@pytest.mark.parametrize("P", [257, 577])
@pytest.mark.parametrize("branch", sorted(BRANCHES))
def test_native_every_branch_of_the_tail(branch, P):
    from d3ga_amd import cage_deform as cd
    kw = dict(BRANCHES[branch])
    merge = kw.pop("merge", True)
    was = cd._merge_policy["enabled"]
    cd._merge_policy["enabled"] = merge
    try:
        A, B, inputs, flags = _native_ab(torch.arange(P) * 5, **kw)
    finally:
        cd._merge_policy["enabled"] = was
    assert (A["records"] is None) == (branch == "no_vertex_gradient")
    if branch == "corners":
        assert tuple(A["records"].shape) == (4 * P, 3)
    if branch == "lbs_pose":
        assert A["pose"] is not None and float(A["pose"][0].abs().max()) > 0
    _assert_sides(A, B, inputs, flags, f"{branch} P={P}")


@pytest.mark.parametrize("pattern", ["culled_wavefronts", "all_culled", "one_per_wavefront"])
def test_native_culling(pattern):
    if pattern == "culled_wavefronts":                       # wavefronts 1, 2 and 4 of 6 hold nothing visible, wavefront 5 is partial
        idx = torch.arange(5 * 64 + 17) * 7
        wave = torch.arange(len(idx)) // 64
        cull = (wave == 1) | (wave == 2) | (wave == 4)
    elif pattern == "all_culled":
        idx = torch.arange(300)
        cull = torch.ones(300, dtype=torch.bool)
    else:
        src, cull = _cull_mask_spread(5)
        idx = (torch.arange(5) * 500)[src]
    A, B, inputs, flags = _native_ab(idx, cull=cull, kind="lbs", delta_barys=True, exp=True)
    _assert_sides(A, B, inputs, flags, pattern)
    c = cull.to(DEV)
    for k in ("gb", "gs", "gr"):                             # a culled Gaussian: exact zeros
        assert float(B[k][c].abs().max()) == 0.0, (pattern, k)
    if pattern == "all_culled":
        assert float(B["records"].abs().max()) == 0.0 and float(B["gv"].abs().max()) == 0.0
    else:
        assert float(B["gb"][~c].abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------
# autograd, whole step
# ------------------------------------------------------------------------------------------------------------
def _frame(name):
    import bench
    return bench.Frame(name, torch.device("cuda", 0), 0)


def _step(f, case):
    """One step of `case` on frame f -> (gradients by name, the deform backward's path)."""
    from d3ga_amd import cage_deform as cd
    from d3ga_amd import rasterizer as R
    from d3ga_amd.cage_deform import fem_energy, lbs_cage_deform
    from d3ga_amd.renderer import render, render_l1, render_pair
    p = f.params
    for t in p.values():
        t.grad = None
    extra = {}
    if case == "fem":
        means, cov6, tp = lbs_cage_deform(f.canon, p["delta_node"], f.joint_mats, f.skin_idx, f.skin_w, f.tetras, f.tetra_id, f.barys0,
                                          f.canon_grad, p["scaling"], p["rotation"], delta_barys=p["delta_bary"], scale_activation="exp")
        pkg = {"means3D": means, "cov3D_precomp": cov6, "opacity_logits": p["opacity"], "shs": p["features"], "rgb": None, "sh_degree": f.sh_degree}
        Dn = torch.linalg.inv(f.canon[f.tetras.long()][:, 1:] - f.canon[f.tetras.long()][:, :1]).contiguous()
        loss = render_l1(f.batch, pkg, f.bg, f.target)["l1"] + 1e-3 * fem_energy(tp, f.tetras, Dn).mean()
    else:
        pkg = f.upstream()
        if case == "second_consumer":
            loss = render_l1(f.batch, pkg, f.bg, f.target)["l1"] + 1e-3 * (pkg["means3D"].sin().sum() + pkg["cov3D_precomp"].cos().sum()) / pkg["means3D"].shape[0]
        elif case == "silhouette_reuse":
            sil = torch.ones(pkg["means3D"].shape[0], 3, device=DEV)
            with R.geometry_reuse():
                a = render(f.batch, pkg, f.bg)["render"]
                b = render(f.batch, pkg, torch.zeros(3, device=DEV), colors_precomp=sil)["render"]
            loss = (a - f.target).abs().mean() + 0.1 * b.mean()
        elif case == "pair":
            sil = torch.ones(pkg["means3D"].shape[0], 3, device=DEV)
            o = render_pair(f.batch, pkg, f.bg, sil, torch.zeros(3, device=DEV))
            loss = (o["render"] - f.target).abs().mean() + 0.1 * o["render2"].mean()
        elif case == "retain_grad":
            pkg["means3D"].retain_grad()
            loss = render_l1(f.batch, pkg, f.bg, f.target)["l1"]
            extra["means"] = pkg["means3D"]
        elif case == "late_retain_grad":                 # asked for between the render and its backward: the claim ends there
            loss = render_l1(f.batch, pkg, f.bg, f.target)["l1"]
            pkg["means3D"].retain_grad()
            extra["means"] = pkg["means3D"]
        else:
            loss = render_l1(f.batch, pkg, f.bg, f.target)["l1"]
    loss.backward()
    torch.cuda.synchronize()
    g = {k: t.grad.detach().clone() for k, t in p.items() if t.grad is not None}
    if "means" in extra:
        g["means"] = extra["means"].grad.detach().clone()
    return g, cd.last_backward_path()


# (a second render of the package revokes the first one's claim: both take the two-kernel path)
CASES = {"single": "fused-tail", "second_consumer": "kernel+deposit", "fem": "fused-tail", "silhouette_reuse": "kernel",
         "pair": "fused-tail", "retain_grad": "kernel", "late_retain_grad": "kernel", "fusion_off": "kernel"}


@pytest.mark.parametrize("scene", ["T1", "C1"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_autograd_whole_step(case, scene):
    """The bar per gradient: 8 x the unfused side's own spread over five runs, at most 2e-2 of its largest element.  A sixth unfused
    run is held to the same bar first -- the inputs must be ones for which the unfused side passes against itself.  (Where the
    five runs agree bit for bit the bar is bit-identity, for the sixth run and for the fused side alike.)"""
    from d3ga_amd import cage_deform as cd
    f = _frame(scene)
    cd.set_render_fusion(False)
    try:
        runs = [_step(f, case) for _ in range(6)]
    finally:
        cd.set_render_fusion(True)
    assert all(path == "kernel" for _, path in runs)
    ref, sixth = runs[0][0], runs[5][0]
    spread = {k: max(float((r[k] - ref[k]).abs().max()) for r, _ in runs[1:5]) for k in ref}
    for k in ref:
        own = float((sixth[k] - ref[k]).abs().max())
        assert own <= min(8.0 * spread[k], 2e-2 * float(ref[k].abs().max())), ("the unfused side against itself", case, k, own, spread[k])
    if case == "fusion_off":
        cd.set_render_fusion(False)
    try:
        got, path = _step(f, case)
    finally:
        cd.set_render_fusion(True)
    assert path == CASES[case], (case, path)
    assert set(got) == set(ref)
    for k in ref:
        top = float(ref[k].abs().max())
        assert top > 0, k
        err = float((got[k] - ref[k]).abs().max())
        print(f"{scene} {case} {k}: |fused - unfused| {err:.3e}, unfused spread over 5 runs {spread[k]:.3e}, largest element {top:.3e}")
        assert err <= min(8.0 * spread[k], 2e-2 * top), (case, k, err, spread[k], top)


def test_a_binding_with_a_second_consumer_is_not_claimed_again():
    """kernel + tails on the deposit + the sums cost more launches than the fusion saves: after one such backward the binding's
    renders go the two-kernel way until set_render_fusion() re-arms them."""
    from d3ga_amd import cage_deform as cd
    f = _frame("T1")
    cd.set_render_fusion(True)
    try:
        assert _step(f, "second_consumer")[1] == "kernel+deposit"
        assert _step(f, "second_consumer")[1] == "kernel" and _step(f, "single")[1] == "kernel"
        cd.set_render_fusion(True)
        assert _step(f, "single")[1] == "fused-tail"
    finally:
        cd.set_render_fusion(True)


def test_intermediate_gradient_of_a_claimed_pair_is_refused():
    from d3ga_amd.renderer import render_l1
    f = _frame("T1")
    pkg = f.upstream()
    loss = render_l1(f.batch, pkg, f.bg, f.target)["l1"]
    with pytest.raises(RuntimeError):
        torch.autograd.grad(loss, pkg["means3D"])


def test_captured_step_replays_the_fused_tail():
    """d3ga_amd.graph capture of the fused step, three replays with different cameras, against eager (the bars of
    tests/test_gpu_view_sharded.py's eager-against-replay check: 1e-5 of the largest element)."""
    from d3ga_amd import cage_deform as cd
    from d3ga_amd import rasterizer as R
    from d3ga_amd.graph import CapturedStep
    f = _frame("T1")
    views = f.camera_cycle()
    params = list(f.params.values())
    eager, dmax = [], 0
    for v in (1, 2, 3):
        f.target_slot.set(views[v][1])           # (staged on the host: the camera's copy below carries the address along)
        f.slot.set(views[v][0])
        for p in params:
            p.grad = None
        f.step()
        torch.cuda.synchronize()
        assert cd.last_backward_path() == "fused-tail"
        eager.append([p.grad.clone() for p in params])
        dmax = max(dmax, R.last_counters()["D"])
    R.set_capacity_policy("static", int(1.5 * dmax) + 1024)
    try:
        for p in params:
            p.grad = None
        cap = CapturedStep(f.step, params=params, camera=f.slot, slots={"target": f.target_slot})
        for j, v in enumerate((1, 2, 3)):
            cap.replay(camera=views[v][0], target=views[v][1])
            torch.cuda.synchronize()
            err = max(float((p.grad - r).abs().max() / (r.abs().max() + 1e-30)) for p, r in zip(params, eager[j]))
            assert err < 1e-5, (v, err)
    finally:
        R.set_capacity_policy("auto")
