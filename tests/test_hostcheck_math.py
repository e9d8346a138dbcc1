"""The product's per-element arithmetic headers (d3ga_math.h, raster_pre_body.h -- the very code the gfx950
kernels execute per Gaussian -- and body_model_math.h, the body model's per-joint math), compiled for the host, against the
oracle.  Runs without a GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT, ptr
from oracle import deform as od
from oracle import raster_c as rc
from oracle import raster_torch as rt
from util import elementwise_excess, rel_err, scene_inputs

from d3ga_amd._lib import RasterParams


def _np(t):
    return np.ascontiguousarray(t.detach().numpy())


def test_deform_forward_backward_vs_golden(hostcheck, golden):
    for name in ("deform_case0.npz", "deform_case1.npz"):
        g = golden(name)
        P, V = g["tetra_id"].shape[0], g["tetpoints"].shape[0]
        tets, tid = g["tetras"].astype(np.int32), g["tetra_id"].astype(np.int32)
        tp, barys = g["tetpoints"], g["canon_barys"]
        cg = np.ascontiguousarray(g["canonical_gradient"])
        scales, rots = g["scales"], g["rotations"]
        means, cov6 = np.zeros((P, 3), np.float32), np.zeros((P, 6), np.float32)
        hostcheck.hc_deform_fwd(P, ptr(tp), ptr(tets), ptr(tid), ptr(barys), ptr(cg), ptr(scales), ptr(rots), ptr(means),
                                ptr(cov6))
        np.testing.assert_allclose(means, g["means3D"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(cov6, g["cov3D_precomp"], rtol=5e-4, atol=1e-10)
        # backward w.r.t. (tetpoints, barys, activated scales, normalised rotation) vs oracle autograd
        t = lambda a: torch.from_numpy(a).double().requires_grad_(True)
        tp_t, b_t, s_t, r_t = t(tp), t(barys), t(scales), t(rots)
        m, c = od.cage_deform(tp_t, torch.from_numpy(tets), torch.from_numpy(tid), b_t, torch.from_numpy(cg).double(),
                              s_t, r_t)
        gm, gc = g["up_grad_means"], g["up_grad_cov"]
        ((m * torch.from_numpy(gm).double()).sum() + (c * torch.from_numpy(gc).double()).sum()).backward()
        g_tp, g_b = np.zeros((V, 3), np.float32), np.zeros((P, 4), np.float32)
        g_s, g_r = np.zeros((P, 3), np.float32), np.zeros((P, 4), np.float32)
        hostcheck.hc_deform_bwd(P, V, ptr(tp), ptr(tets), ptr(tid), ptr(barys), ptr(cg), ptr(scales), ptr(rots), ptr(gm),
                                ptr(gc), ptr(g_tp), ptr(g_b), ptr(g_s), ptr(g_r))
        assert rel_err(g_tp, _np(tp_t.grad)) < 1e-4
        assert rel_err(g_b, _np(b_t.grad)) < 1e-5
        assert rel_err(g_s, _np(s_t.grad)) < 1e-4
        assert rel_err(g_r, _np(r_t.grad)) < 1e-4
        # the reference's own gradient w.r.t. tetpoints and barys (captured by tools/gen_golden.py)
        assert rel_err(g_tp, g["grad_tetpoints"]) < 1e-3
        assert rel_err(g_b, g["grad_barys"]) < 1e-3


def test_fem_energy_vs_oracle(hostcheck, golden):
    g = golden("deform_case0.npz")
    T, V = g["tetras"].shape[0], g["tetpoints"].shape[0]
    tets, tp, Dn = g["tetras"].astype(np.int32), g["tetpoints"], np.ascontiguousarray(g["Dn_inv"])
    e = np.zeros(T, np.float32)
    hostcheck.hc_fem_fwd(T, ptr(tp), ptr(tets), ptr(Dn), ptr(e))
    tp_t = torch.from_numpy(tp).double().requires_grad_(True)
    ref = od.fem_energy(tp_t, torch.from_numpy(tets), torch.from_numpy(Dn).double())
    np.testing.assert_allclose(e, _np(ref), rtol=1e-3, atol=1e-5)
    np.testing.assert_allclose(e.mean(), g["fm_energy"][0], rtol=1e-4)
    w = np.random.default_rng(0).normal(size=T).astype(np.float32)
    (ref * torch.from_numpy(w).double()).sum().backward()
    gt = np.zeros((V, 3), np.float32)
    hostcheck.hc_fem_bwd(T, V, ptr(tp), ptr(tets), ptr(Dn), ptr(w), ptr(gt))
    assert rel_err(gt, _np(tp_t.grad)) < 1e-4


def _prm(inp, M, deg, mod=1.0, antialiasing=0):
    return RasterParams(P=inp["means3D"].shape[0], M=M, sh_degree=deg, W=inp["W"], H=inp["H"],
                        tanfovx=inp["cam"]["tanfovx"], tanfovy=inp["cam"]["tanfovy"], scale_modifier=mod,
                        antialiasing=antialiasing, prefiltered=0, debug=0)


def _run_pre(hostcheck, inp, prm, shs=None, colors=None, cov=None, scales=None, rots=None):
    P = prm.P
    o = dict(depth=np.zeros(P, np.float32), xy=np.zeros((P, 2), np.float32), conic_o=np.zeros((P, 4), np.float32),
             rgb=np.zeros((P, 3), np.float32), radii=np.zeros(P, np.int32), rect=np.zeros((P, 4), np.int32),
             clamped=np.zeros(P, np.uint8), cov3D=np.zeros((P, 6), np.float32))
    hostcheck.hc_preprocess(ctypes.byref(prm), ptr(_np(inp["means3D"])), ptr(shs), ptr(colors), ptr(_np(inp["opacities"])),
                            ptr(scales), ptr(rots), ptr(cov), ptr(_np(inp["view"])), ptr(_np(inp["proj"])),
                            ptr(_np(inp["campos"])), ptr(o["depth"]), ptr(o["xy"]), ptr(o["conic_o"]), ptr(o["rgb"]),
                            ptr(o["radii"]), ptr(o["rect"]), ptr(o["clamped"]), ptr(o["cov3D"]))
    return o


def test_preprocess_forward_vs_oracles(hostcheck):
    inp = scene_inputs("T1", scale_mult=3.0)
    prm = _prm(inp, 16, 3)
    shs, cov = _np(inp["shs"]), _np(inp["cov6"])
    o = _run_pre(hostcheck, inp, prm, shs=shs, cov=cov)
    cam = inp["cam"]
    _, radii, _, ctx = rc.forward(_np(inp["means3D"]), _np(inp["opacities"]), np.ones(3, np.float32),
                                  cam["world_view_transform"], cam["full_proj_transform"], cam["camera_center"],
                                  cam["tanfovx"], cam["tanfovy"], inp["W"], inp["H"], cov3D_precomp=cov, shs=shs,
                                  sh_degree=3)
    g = rc.geom(ctx)
    np.testing.assert_array_equal(o["radii"], radii)
    vis = radii > 0
    assert vis.sum() > 100
    np.testing.assert_allclose(o["depth"][vis], g["depth"][vis], rtol=1e-6)
    np.testing.assert_allclose(o["xy"][vis], g["xy"][vis], rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(o["conic_o"][vis], g["conic_o"][vis], rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(o["rgb"][vis], g["rgb"][vis], rtol=1e-5, atol=1e-6)
    # tile rectangles vs the dense torch oracle
    pre = rt.preprocess(inp["means3D"], inp["opacities"], inp["view"], inp["proj"], inp["campos"], cam["tanfovx"],
                        cam["tanfovy"], inp["W"], inp["H"], cov3D_precomp=inp["cov6"], shs=inp["shs"], sh_degree=3)
    rect = np.stack([r.numpy() for r in pre["rect"]], 1)
    np.testing.assert_array_equal(o["rect"][vis], rect[vis])


def _bwd_case(hostcheck, inp, prm, use_sh, from_sr, seed, invdepth=False, use_dcol=False):
    """Feed the same accumulated screen-space gradients to the product's per-Gaussian backward and to an
    autograd evaluation of the oracle's preprocess stage."""
    P = prm.P
    rng = np.random.default_rng(seed)
    shs = _np(inp["shs"]) if use_sh else None
    colors = None if use_sh else _np(inp["rgb"])
    q = torch.nn.functional.normalize(inp["scene"]["rotation"]) * 1.1       # deliberately not unit norm
    scales, rots = (_np(inp["scales"]), _np(q)) if from_sr else (None, None)
    cov = None if from_sr else _np(inp["cov6"])
    o = _run_pre(hostcheck, inp, prm, shs=shs, colors=colors, cov=cov, scales=scales, rots=rots)
    vis = o["radii"] > 0
    acc = np.zeros((P, 16), np.float32)       # D3GA_ACC_STRIDE
    acc[:, [0, 1, 3, 4, 5, 6, 7, 8, 9]] = rng.normal(size=(P, 9)).astype(np.float32)
    if invdepth:
        acc[:, 10] = rng.normal(size=P).astype(np.float32)
    acc[~vis] = 0
    outs = dict(m3=np.zeros((P, 3), np.float32), m2=np.zeros((P, 3), np.float32), op=np.zeros((P, 1), np.float32),
                sh=np.zeros((P, 16, 3), np.float32) if use_sh else None,
                col=None if use_sh else np.zeros((P, 3), np.float32),
                cov=None if from_sr else np.zeros((P, 6), np.float32),
                sc=np.zeros((P, 3), np.float32) if from_sr else None, ro=np.zeros((P, 4), np.float32) if from_sr else None)
    hostcheck.hc_preprocess_bwd(ctypes.byref(prm), ptr(_np(inp["means3D"])), ptr(shs), ptr(scales), ptr(rots),
                                ptr(_np(inp["view"])), ptr(_np(inp["proj"])), ptr(_np(inp["campos"])), ptr(o["radii"]),
                                ptr(o["cov3D"]), ptr(o["clamped"]), ptr(acc), ptr(outs["m3"]), ptr(outs["m2"]),
                                ptr(outs["op"]), ptr(outs["sh"]), ptr(outs["col"]), ptr(outs["cov"]), ptr(outs["sc"]),
                                ptr(outs["ro"]), ptr(np.ascontiguousarray(o["conic_o"][:, 3])), int(use_dcol))
    if use_sh and not use_dcol:       # round 5: the same case with d(colour)/d(direction) from the forward instead of the coefficients
        _bwd_case(hostcheck, inp, prm, use_sh, from_sr, seed, invdepth, use_dcol=True)
    # oracle: autograd through preprocess with a linear functional reproducing `acc`
    dd = torch.float64
    m = inp["means3D"].to(dd).requires_grad_(True)
    kw = {}
    if from_sr:
        s_t = torch.from_numpy(scales).to(dd).requires_grad_(True)
        r_t = torch.from_numpy(rots).to(dd).requires_grad_(True)
        kw.update(scales=s_t, rotations=r_t, scale_modifier=prm.scale_modifier)
    else:
        c_t = inp["cov6"].to(dd).requires_grad_(True)
        kw.update(cov3D_precomp=c_t)
    if use_sh:
        sh_t = inp["shs"].to(dd).requires_grad_(True)
        kw.update(shs=sh_t, sh_degree=prm.sh_degree)
    else:
        col_t = inp["rgb"].to(dd).requires_grad_(True)
        kw.update(colors_precomp=col_t)
    op_t = inp["opacities"].to(dd).requires_grad_(True)
    pre = rt.preprocess(m, op_t, inp["view"], inp["proj"], inp["campos"], prm.tanfovx, prm.tanfovy,
                        prm.W, prm.H, antialiasing=bool(prm.antialiasing), **kw)
    a = torch.from_numpy(acc).to(dd)
    # mean2D gradient is expressed in NDC-scaled units: d(pixel)/d(ndc) = 0.5*W  => pixel-space grad = a / (0.5 W)
    L = (pre["xy"][:, 0] * a[:, 0] / (0.5 * prm.W)).sum() + (pre["xy"][:, 1] * a[:, 1] / (0.5 * prm.H)).sum()
    L = L + (pre["conic"][:, 0] * a[:, 3]).sum() + (pre["conic"][:, 1] * 2.0 * a[:, 4]).sum() + (pre["conic"][:, 2] * a[:, 5]).sum()
    L = L + (pre["rgb"] * a[:, 7:10]).sum() + (pre["opacity"] * a[:, 6]).sum()
    if invdepth:
        visible = torch.from_numpy(vis)
        L = L + ((1.0 / pre["depth"][visible]) * a[visible, 10]).sum()
    L.backward()
    assert rel_err(outs["m3"], _np(m.grad)) < 1e-3
    if use_sh:
        assert rel_err(outs["sh"], _np(sh_t.grad)) < 1e-4
    else:
        assert rel_err(outs["col"], _np(col_t.grad)) < 1e-5
    if from_sr:
        assert rel_err(outs["sc"], _np(s_t.grad)) < 1e-3
        assert rel_err(outs["ro"], _np(r_t.grad)) < 1e-3
    else:
        assert rel_err(outs["cov"], _np(c_t.grad)) < 1e-3
    np.testing.assert_array_equal(outs["m2"][:, :2], acc[:, :2])
    if prm.antialiasing:
        assert rel_err(outs["op"][:, 0], _np(op_t.grad).reshape(-1)) < 1e-5
    else:
        np.testing.assert_array_equal(outs["op"][:, 0], acc[:, 6])


def test_preprocess_backward_sh_precomputed_cov(hostcheck):
    inp = scene_inputs("T1", scale_mult=3.0)
    _bwd_case(hostcheck, inp, _prm(inp, 16, 3), use_sh=True, from_sr=False, seed=1)
    _bwd_case(hostcheck, inp, _prm(inp, 16, 1), use_sh=True, from_sr=False, seed=2)


def test_preprocess_backward_colors_scale_rot(hostcheck):
    inp = scene_inputs("T1", scale_mult=3.0)
    _bwd_case(hostcheck, inp, _prm(inp, 0, 0, mod=1.3), use_sh=False, from_sr=True, seed=3)


def test_preprocess_backward_antialiasing_and_inverse_depth(hostcheck):
    """Branch dr_aa: the opacity seen by compositing is opacity x sqrt(max(2.5e-5, det / det_dilated)) -- its chain into
    cov3D / mean / opacity -- and acc[10] = dL/d(1/z) chains into the mean.  Small Gaussians (scale_mult 0.3) put the
    factor well below one; large ones leave it near one."""
    for mult, seed in ((0.3, 5), (3.0, 6)):
        inp = scene_inputs("T1", scale_mult=mult)
        _bwd_case(hostcheck, inp, _prm(inp, 16, 2, antialiasing=1), use_sh=True, from_sr=False, seed=seed, invdepth=True)
        _bwd_case(hostcheck, inp, _prm(inp, 0, 0, mod=1.2, antialiasing=1), use_sh=False, from_sr=True, seed=seed + 10,
                  invdepth=True)
    # forward: the stored opacity is the product
    inp = scene_inputs("T1", scale_mult=0.3)
    prm = _prm(inp, 16, 3, antialiasing=1)
    o = _run_pre(hostcheck, inp, prm, shs=_np(inp["shs"]), cov=_np(inp["cov6"]))
    pre = rt.preprocess(inp["means3D"].double(), inp["opacities"].double(), inp["view"], inp["proj"], inp["campos"],
                        prm.tanfovx, prm.tanfovy, prm.W, prm.H, cov3D_precomp=inp["cov6"].double(), shs=inp["shs"].double(),
                        sh_degree=3, antialiasing=True)
    vis = o["radii"] > 0
    ratio = o["conic_o"][vis, 3] / _np(inp["opacities"]).reshape(-1)[vis]
    assert ratio.min() < 0.5 and ratio.max() <= 1.0
    np.testing.assert_allclose(o["conic_o"][vis, 3], _np(pre["opacity"])[vis], rtol=2e-4)


def test_preprocess_backward_with_clamped_sh_and_frustum_edge(hostcheck):
    """Dark SH colours (clamp mask active) and a camera so close that x/z, y/z leave the 1.3*tanfov guard band."""
    inp = scene_inputs("T1", scale_mult=3.0, azimuth=1.2)
    inp["shs"] = inp["shs"].clone()
    inp["shs"][::2, 0, :] = -2.5           # SH_C0 * (-2.5) + 0.5 < 0  -> clamped
    prm = _prm(inp, 16, 2)
    prm.tanfovx *= 0.25                    # narrow guard band: many Gaussians are clamped in x
    _bwd_case(hostcheck, inp, prm, use_sh=True, from_sr=False, seed=4)


def _views_records(hostcheck, prm, views, rng, means, cov=None, scales=None, rots=None, shs=None, colors=None):
    """Forward records of k views (record j = v P + i) as preprocess leaves them, plus seeded accumulator and dcol planes."""
    P, k = prm.P, len(views)
    rect, clamped, conic_o, cov3D = (np.zeros((k * P, 2), np.uint32), np.zeros(k * P, np.uint8), np.zeros((k * P, 4), np.float32),
                                     np.zeros((k * P, 6), np.float32))
    for v, inp in enumerate(views):
        sl = slice(v * P, (v + 1) * P)
        o = _run_pre(hostcheck, dict(inp, means3D=torch.from_numpy(means[v])), prm, shs=shs, colors=colors, cov=cov[v] if cov is not None else None,
                     scales=scales[v] if scales is not None else None, rots=rots[v] if rots is not None else None)
        r = o["rect"].astype(np.uint32)
        rect[sl] = np.stack([r[:, 0] | (r[:, 1] << 16), r[:, 2] | (r[:, 3] << 16)], 1)
        clamped[sl], conic_o[sl], cov3D[sl] = o["clamped"], o["conic_o"], o["cov3D"]
    rect[rng.random(k * P) < 0.3] = 0                  # culled in that view (an empty rectangle), visible in others
    acc = rng.normal(size=(k * P, 16)).astype(np.float32)
    acc[:, [2, 11, 12, 13, 14, 15]] = 0
    dcol = rng.normal(size=(9, k * P)).astype(np.float32)
    return rect, acc, clamped, conic_o, cov3D, dcol


def test_preprocess_backward_views_body_matches_single_view(hostcheck):
    """The view-batched backward's per-Gaussian walk against k calls of the single-view backward, views added in ascending
    order as the per-view launches add them.  Both form the same sums in the same order (no contraction on the host): every
    gradient is bit-identical, except (scale, rotation), which the walk maps ONCE from the summed covariance gradient while the
    single-view calls map every view's and add -- a linear map applied before or after a float sum, so those two differ by
    rounding only: within 1e-5 of the largest element."""
    f = ctypes.c_float
    cases = [dict(k=3, sh=True), dict(k=4, sh=False, sr=True), dict(k=2, sh=False, frames=True, sr=True),
             dict(k=3, sh=False, pva=True), dict(k=5, sh=True, frames=True)]
    for n, c in enumerate(cases):
        k, sh, sr, frames, pva = c["k"], c["sh"], c.get("sr", False), c.get("frames", False), c.get("pva", False)
        views = [scene_inputs("T1", scale_mult=2.0, azimuth=0.4 + 0.9 * v) for v in range(k)]
        inp = views[0]
        prm = _prm(inp, 16 if sh else 0, 3 if sh else 0, mod=1.1)
        prm.n_views, prm.per_view_geometry, prm.per_view_appearance = k, int(frames), int(pva)
        P, rng = prm.P, np.random.default_rng(20 + n)
        kg = k if frames else 1                                    # geometry records (a batch of frames: one per view)
        means = np.stack([_np(inp["means3D"]) + (0.02 * v * rng.normal(size=(P, 3)).astype(np.float32) if frames else 0)
                          for v in range(k)]).astype(np.float32)
        q = _np(torch.nn.functional.normalize(inp["scene"]["rotation"]))
        scales = np.stack([_np(inp["scales"])] * k) if sr else None
        rots = np.stack([q] * k) if sr else None
        cov = None if sr else np.stack([_np(inp["cov6"])] * k)
        shs = _np(inp["shs"]) if sh else None
        rect, acc, clamped, conic_o, cov3D, dcol = _views_records(hostcheck, prm, views, rng, means, cov=cov, scales=scales, rots=rots,
                                                                  shs=shs, colors=None if sh else _np(inp["rgb"]))
        vis = (rect[:, 1] & 0xffff) > (rect[:, 0] & 0xffff)
        assert vis.any() and not vis.all() and (vis.reshape(k, P).any(0) & ~vis.reshape(k, P).all(0)).any()   # culled in some views only
        cov6 = np.ascontiguousarray((cov.reshape(-1, 6) if cov is not None else cov3D)[: kg * P])
        view = np.stack([_np(x["view"]) for x in views]); proj = np.stack([_np(x["proj"]) for x in views])
        campos = np.stack([_np(x["campos"]) for x in views])
        na = k if pva else 1                                       # appearance gradient records
        def outs():
            return dict(m3=np.zeros((kg * P, 3), np.float32), m2=np.zeros((k * P, 3), np.float32), op=np.zeros(na * P, np.float32),
                        sh=np.zeros((P, 16, 3), np.float32) if sh else None, col=None if sh else np.zeros((na * P, 3), np.float32),
                        cov=None if sr else np.zeros((kg * P, 6), np.float32),
                        sc=np.zeros((kg * P, 3), np.float32) if sr else None, ro=np.zeros((kg * P, 4), np.float32) if sr else None)
        a = outs()
        hostcheck.hc_preprocess_bwd_views(ctypes.byref(prm), k, ptr(means), ptr(cov6), ptr(scales), ptr(rots), ptr(view), ptr(proj),
                                          ptr(campos), 3, ptr(rect), ptr(acc), ptr(clamped), ptr(conic_o), ptr(dcol), int(sh),
                                          ctypes.c_int64(P if frames else 0), int(pva), ptr(a["m3"]), ptr(a["m2"]), ptr(a["op"]),
                                          ptr(a["sh"]), ptr(a["col"]), ptr(a["cov"]), ptr(a["sc"]), ptr(a["ro"]))
        b = outs()
        sh_sum = np.zeros((P, 16, 3), np.float32)
        for v in range(k):
            g, ap = (v if frames else 0) * P, (v if pva else 0) * P      # geometry / appearance record offsets
            row = np.zeros((P, 16, 3), np.float32) if sh else None
            def o(x, n, off):
                return None if x is None else ptr(x[off:]) if n == 1 else x[off:].ctypes.data_as(ctypes.c_void_p)
            accum = 0 if v == 0 else (0 if pva else 1) | (0 if frames else 2)
            hostcheck.hc_preprocess_bwd_view(ctypes.byref(prm), k, v, ptr(means[v]), ptr(cov6[g:]), ptr(scales[v] if sr else None),
                                             ptr(rots[v] if sr else None), ptr(view[v]), ptr(proj[v]), ptr(campos[v]), ptr(rect), ptr(acc),
                                             ptr(clamped), ptr(conic_o), ptr(dcol) if sh else None, ptr(shs), o(b["m3"], 3, g),
                                             o(b["m2"], 3, v * P), o(b["op"], 1, ap), ptr(row), o(b["col"], 3, ap), o(b["cov"], 6, g),
                                             o(b["sc"], 3, g), o(b["ro"], 4, g), accum)
            if sh:
                sh_sum += row
        b["sh"] = sh_sum if sh else None
        for key in ("m3", "m2", "op", "sh", "col", "cov"):
            if a[key] is not None:
                np.testing.assert_array_equal(a[key], b[key], err_msg=f"case {c}: {key}")
        if sr:
            for key in ("sc", "ro"):
                assert rel_err(a[key], b[key]) < 1e-5, (c, key, rel_err(a[key], b[key]))


@pytest.fixture(scope="module")
def hostcheck_body():
    """hostcheck.cpp built as the shared `hostcheck` fixture builds it, but rebuilt when body_model_math.h changes too (the
    shared fixture does not watch that header)."""
    src = os.path.join(ROOT, "tests", "hostcheck", "hostcheck.cpp")
    out_dir = os.path.join(ROOT, "tests", "hostcheck", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libhostcheck_body.so")
    deps = [src] + [os.path.join(ROOT, "d3ga_amd", "csrc", h) for h in ("d3ga_math.h", "raster_pre_body.h", "body_model_math.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", so])
    return ctypes.CDLL(so)


def _edge_rotations(seed):
    from smplx_ref import EDGE_ANGLES, edge_rotations
    return edge_rotations(np.random.default_rng(seed), 4 * 3 * len(EDGE_ANGLES))


def test_body_rodrigues_forward_over_the_angle_edges(hostcheck_body):
    """bm::rodrigues against the float64 oracle at the float32 inputs: exact zero, 1e-7 .. 1e-3, pi, 2 pi and beyond, on
    random and coordinate axes.  Bar: 4 float32 ulps of max(1, |theta|) per entry (t carries |theta|'s rounding into sin)."""
    from smplx_ref import rodrigues
    r = _edge_rotations(0)
    n = len(r)
    R = np.zeros((n, 9), np.float32)
    hostcheck_body.hc_body_rodrigues(n, ptr(r), ptr(R))
    want = rodrigues(torch.from_numpy(r).double()).reshape(n, 9).numpy()
    t = np.linalg.norm(r.astype(np.float64) + 1e-8, axis=1)
    err = np.abs(R - want).max(1) / (2.0 ** -23 * np.maximum(1.0, t))
    i = int(np.argmax(err))
    assert err[i] <= 4.0, f"rodrigues: {err[i]:.2f} ulps at theta = {r[i]}"
    assert np.all(R[np.linalg.norm(r, axis=1) == 0] == np.eye(3, dtype=np.float32).reshape(9)), "rodrigues(0) != I"


def test_body_rodrigues_backward_over_the_angle_edges(hostcheck_body):
    """bm::rodrigues_bwd against float64 autograd of the oracle's rodrigues (same 1e-8 offset), per rotation: the
    element-wise bar, and the row's largest error within 2e-5 of its largest element (1.9e-6 measured, at 2 pi)."""
    from smplx_ref import rodrigues
    r = _edge_rotations(1)
    n = len(r)
    G = np.random.default_rng(2).normal(size=(n, 9)).astype(np.float32)
    dr = np.zeros((n, 3), np.float32)
    hostcheck_body.hc_body_rodrigues_bwd(n, ptr(r), ptr(G), ptr(dr))
    rt = torch.from_numpy(r).double().requires_grad_(True)
    (rodrigues(rt).reshape(n, 9) * torch.from_numpy(G).double()).sum().backward()
    want = rt.grad.numpy()
    assert np.isfinite(dr).all()
    for i in range(n):
        ex = elementwise_excess(dr[i], want[i])
        rel = float(np.abs(dr[i] - want[i]).max() / np.abs(want[i]).max())
        assert ex <= 1.0 and rel <= 2e-5, f"rodrigues_bwd at theta = {r[i]}: x{ex:.2f} of the bar, row error {rel:.2e}"


def test_body_compose_matches_float64(hostcheck_body):
    rng = np.random.default_rng(3)
    n = 64
    from smplx_ref import rodrigues
    Rp = rodrigues(torch.from_numpy(rng.normal(size=(n, 3)))).numpy().astype(np.float32).reshape(n, 9)
    R = rodrigues(torch.from_numpy(rng.normal(size=(n, 3)))).numpy().astype(np.float32).reshape(n, 9)
    tp, t = (rng.normal(size=(n, 3)).astype(np.float32) for _ in range(2))
    Ro, to = np.zeros((n, 9), np.float32), np.zeros((n, 3), np.float32)
    hostcheck_body.hc_body_compose(n, ptr(Rp), ptr(tp), ptr(R), ptr(t), ptr(Ro), ptr(to))
    Rp64, R64 = Rp.astype(np.float64).reshape(n, 3, 3), R.astype(np.float64).reshape(n, 3, 3)
    want_R = (Rp64 @ R64).reshape(n, 9)
    want_t = np.einsum("nij,nj->ni", Rp64, t.astype(np.float64)) + tp
    assert np.abs(Ro - want_R).max() <= 4 * 2.0 ** -23
    assert np.abs(to - want_t).max() <= 8 * 2.0 ** -23 * np.abs(want_t).max()
