"""The per-Gaussian kernels at the shapes where their paths part (preprocess_kernel's full wavefronts of the training forward
project and reserve their list slots before the SH passes and load the mean once; partial wavefronts, the forward-only kernels and
precomputed colours keep the other order).  Only the schedule differs between the paths, so the claims are the ones the kernels
always had: tile offsets, sorted lists, counters and radii are the C oracle's bit for bit, images are bit-identical to a render of
the same Gaussians laid out one per wavefront and at another index offset (full against partial wavefronts), gradients meet the
bars of tests/test_gpu_parity.py, and the cage deformation meets the bars of the existing cage tests against oracle/deform.py at
the Gaussian counts around a workgroup, in both gradient layouts and both routes of the vertex gradient.

Shapes: a 64 x 48 raster, SH degree 3 (M = 16), P in {1, 65, 209, 257}: 209 = three full wavefronts on the fast path and one
partial on the generic path in one launch, 257 = a second workgroup holding one Gaussian; and a 16 x 16 raster (one tile) at P = 65.  SEEDS names the scene seed of every P:
chosen on the CPU with the oracle alone so that the Gaussians touching a marginal pixel (tests/util.py: Parity) are at most 5 %."""
import functools

import numpy as np
import pytest
import torch

from oracle import camera as oc
from oracle import deform as od
from oracle import raster_c as rc
from test_gpu_parity import _assert_grads, _oracle as _parity_oracle
from util import Parity, elementwise_excess, rel_err, scene_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
W, H = 64, 48
KEYS = ("means3D", "cov6", "opacities", "shs", "rgb", "scales", "rots")
SEEDS = {1: 17, 65: 17, 209: 17, 257: 17}
MAX_MARGINAL_GAUSSIANS = 0.05


def _np(t):
    return np.ascontiguousarray(t.detach().cpu().numpy())


@functools.lru_cache(maxsize=None)
def _scene(seed, cx=None, cy=None, width=W, height=H):
    inp = scene_inputs("T1", seed=seed, scale_mult=3.0, width=width, height=height, cx=cx, cy=cy)
    inp["rots"] = torch.nn.functional.normalize(inp["scene"]["rotation"])      # (for the covariances formed from scale and rotation)
    return inp


def _take(inp, idx):
    g = {k: inp[k][idx].clone().contiguous() for k in KEYS}
    g["P"] = g["means3D"].shape[0]
    return g


def _gaussians(P, inp=None):
    """P Gaussians spread over the body: every (N // P)-th of the scene"""
    inp = inp or _scene(SEEDS[P])
    n = inp["means3D"].shape[0]
    return _take(inp, torch.arange(P) * max(1, n // (P + 1)))


def _cull(g, mask):
    """Move the Gaussians `mask` behind the camera (seen from azimuth 0.4: 100 m along -z is behind it)."""
    g = dict(g)
    m = g["means3D"].clone()
    m[mask, 2] -= 100.0
    g["means3D"] = m
    return g


def _spread(g):
    """One Gaussian per wavefront (Gaussian i at index 64 i, the rest of its wavefront culled copies): same lists, same image."""
    P = g["P"]
    s = _take(g, torch.arange(64 * P) // 64)
    keep = torch.zeros(64 * P, dtype=torch.bool)
    keep[::64] = True
    return _cull(s, ~keep)


def _shifted(g, k):
    """The same Gaussians behind k culled ones: every Gaussian sits in another lane, the last wavefront is cut elsewhere."""
    s = _take(g, torch.cat([torch.zeros(k, dtype=torch.long), torch.arange(g["P"])]))
    front = torch.zeros(g["P"] + k, dtype=torch.bool)
    front[:k] = True
    return _cull(s, front)


def _settings(inp, bg, sh_degree):
    from d3ga_amd.rasterizer import GaussianRasterizationSettings
    return GaussianRasterizationSettings(
        image_height=inp["H"], image_width=inp["W"], tanfovx=inp["cam"]["tanfovx"], tanfovy=inp["cam"]["tanfovy"], bg=bg.to(DEV),
        scale_modifier=1.0, viewmatrix=inp["view"].to(DEV), projmatrix=inp["proj"].to(DEV), sh_degree=sh_degree,
        campos=inp["campos"].to(DEV), prefiltered=False, debug=False, antialiasing=False)


def _render(g, inp, bg, use_sh=True, train=False, from_sr=False):
    """-> (image, radii, tile_start, point_list, counters); train: the forward that leaves d(colour)/d(direction); from_sr: the
    covariances are formed in the kernel from (scales, rots) instead of read from cov6"""
    from d3ga_amd import rasterizer as R
    rast = R.GaussianRasterizer(_settings(inp, bg, 3 if use_sh else 0))
    t = {k: g[k].to(DEV) for k in KEYS}
    if train:
        t["means3D"].requires_grad_(True)
    with torch.set_grad_enabled(train):
        color, radii, _ = rast(means3D=t["means3D"], means2D=None, opacities=t["opacities"], shs=t["shs"] if use_sh else None,
                               colors_precomp=None if use_sh else t["rgb"],
                               **(dict(scales=t["scales"], rotations=t["rots"]) if from_sr else dict(cov3D_precomp=t["cov6"])))
    start, plist, _ = R.last_tile_lists(inp["W"], inp["H"])
    return color.detach(), radii, start, plist, R.last_counters()


def _oracle(g, inp, bg, use_sh=True, from_sr=False):
    """-> (tile_start, point_list, D, visible, radii) of the C oracle"""
    cam = inp["cam"]
    kw = dict(shs=_np(g["shs"]), sh_degree=3) if use_sh else dict(colors_precomp=_np(g["rgb"]))
    kw.update(dict(scales=_np(g["scales"]), rotations=_np(g["rots"]), scale_modifier=1.0) if from_sr else dict(cov3D_precomp=_np(g["cov6"])))
    _, radii, _, ctx = rc.forward(_np(g["means3D"]), _np(g["opacities"]), _np(bg), cam["world_view_transform"], cam["full_proj_transform"],
                                  cam["camera_center"], cam["tanfovx"], cam["tanfovy"], inp["W"], inp["H"], **kw)
    ostart, olist = rc.tile_lists(ctx)
    return np.asarray(ostart), np.asarray(olist), rc.num_rendered(ctx), int((radii > 0).sum()), np.asarray(radii)


def _assert_lists(out, ref, what=""):
    _, radii, start, plist, cnt = out
    ostart, olist, D, visible, oradii = ref
    np.testing.assert_array_equal(_np(start), ostart, err_msg=f"tile offsets {what}")
    np.testing.assert_array_equal(_np(plist), olist, err_msg=f"sorted lists {what}")
    np.testing.assert_array_equal(_np(radii), oradii, err_msg=f"radii {what}")
    assert (cnt["D"], cnt["overflow"], cnt["visible"]) == (D, False, visible), (what, cnt)
    lengths = np.diff(ostart)
    assert cnt["max_tile"] == (int(lengths.max()) if lengths.size else 0), (what, cnt)


VARIANTS = [("train", True, True), ("forward_only", True, False), ("colors_precomp", False, False)]


@pytest.mark.parametrize("variant,use_sh,train", VARIANTS)
@pytest.mark.parametrize("P", [1, 65, 209, 257])
def test_lists_counters_radii_and_images(P, variant, use_sh, train):
    inp = _scene(SEEDS[P])
    g = _gaussians(P)
    bg = torch.tensor([0.2, 0.4, 0.6])
    out = _render(g, inp, bg, use_sh, train)
    ref = _oracle(g, inp, bg, use_sh)
    assert ref[2] > 0
    _assert_lists(out, ref, f"P={P} {variant}")
    one = _render(_spread(g), inp, bg, use_sh, train)
    assert one[4]["D"] == ref[2] and torch.equal(one[0], out[0]), float((one[0] - out[0]).abs().max())
    np.testing.assert_array_equal(_np(one[3]), 64 * ref[1])


@pytest.mark.parametrize("variant,use_sh,train", VARIANTS)
def test_one_tile_raster(variant, use_sh, train):
    """16 x 16 at P = 65: the grid is ONE tile, so every wavefront's window is 1 x 1 and the whole frame takes one reservation slot
    per wavefront -- a full wavefront and a partial one of one Gaussian add to the same tile."""
    P = 65
    inp = _scene(SEEDS[P], width=16, height=16)
    g = _gaussians(P, inp)
    bg = torch.tensor([0.2, 0.4, 0.6])
    out = _render(g, inp, bg, use_sh, train)
    ref = _oracle(g, inp, bg, use_sh)
    assert ref[0].shape[0] == 2 and ref[2] > 1, "not one tile with several duplicates"
    _assert_lists(out, ref, f"16x16 {variant}")
    one = _render(_spread(g), inp, bg, use_sh, train)
    assert one[4]["D"] == ref[2] and torch.equal(one[0], out[0]), float((one[0] - out[0]).abs().max())
    np.testing.assert_array_equal(_np(one[3]), 64 * ref[1])


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("P", [209, 257])
def test_covariances_from_scale_and_rotation(P, train):
    """The route without cov3D_precomp (full wavefronts of the training forward take the order of the partial ones there): lists,
    counters and radii against the oracle, the image against the layouts one per wavefront and at index offset 17."""
    inp = _scene(SEEDS[P])
    g = _gaussians(P)
    bg = torch.tensor([0.2, 0.4, 0.6])
    out = _render(g, inp, bg, True, train, from_sr=True)
    ref = _oracle(g, inp, bg, True, from_sr=True)
    assert ref[2] > 0
    _assert_lists(out, ref, f"P={P} train={train} scale/rotation")
    one = _render(_spread(g), inp, bg, True, train, from_sr=True)
    assert one[4]["D"] == ref[2] and torch.equal(one[0], out[0]), float((one[0] - out[0]).abs().max())
    np.testing.assert_array_equal(_np(one[3]), 64 * ref[1])
    off = _render(_shifted(g, 17), inp, bg, True, train, from_sr=True)
    assert torch.equal(off[0], out[0]) and torch.equal(off[1][17:], out[1]) and torch.equal(off[3], out[3] + 17)


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("P", [1, 65, 209, 257])
def test_full_against_partial_wavefronts(P, train):
    """The same Gaussians at index offset 0 and 17: image, radii and lists (by Gaussian) must not change in a bit."""
    inp = _scene(SEEDS[P])
    g = _gaussians(P)
    bg = torch.tensor([0.7, 0.1, 0.3])
    a = _render(g, inp, bg, True, train)
    b = _render(_shifted(g, 17), inp, bg, True, train)
    assert torch.equal(a[0], b[0]), float((a[0] - b[0]).abs().max())
    assert torch.equal(a[1], b[1][17:]) and int(b[1][:17].abs().max()) == 0
    assert torch.equal(a[2], b[2]) and torch.equal(a[3] + 17, b[3])


@pytest.mark.parametrize("P", [209, 257])
def test_a_full_wavefront_behind_the_camera_between_visible_ones(P):
    """Wavefront 1 sees nothing: empty window, reservation skipped, its neighbours reserve.  (Three wavefronts at least: not at
    P = 1 and 65.)"""
    inp = _scene(SEEDS[P])
    g = _gaussians(P)
    g = _cull(g, (torch.arange(P) // 64) == 1)
    bg = torch.tensor([0.3, 0.6, 0.1])
    ref = _oracle(g, inp, bg)
    assert 0 < ref[3] <= P - 64 and int(ref[4][64:128].max()) == 0
    for train in (True, False):
        out = _render(g, inp, bg, True, train)
        _assert_lists(out, ref, f"P={P} train={train}")
        assert torch.equal(_render(_spread(g), inp, bg, True, train)[0], out[0])


@pytest.mark.parametrize("P", [1, 65, 209, 257])
def test_windowed_camera_slot(P):
    """An off-centre principal point: the window render is the padded render cropped, bit for bit, in both kernel variants."""
    from d3ga_amd.renderer import render
    inp = _scene(SEEDS[P], cx=23, cy=31)
    g = _gaussians(P, inp)
    bg = torch.tensor([0.3, 0.6, 0.1], device=DEV)
    imgs = []
    for train in (False, True):
        pkg = {"means3D": g["means3D"].to(DEV).requires_grad_(train), "cov3D_precomp": g["cov6"].to(DEV), "opacities": g["opacities"].to(DEV),
               "shs": g["shs"].to(DEV), "rgb": None, "sh_degree": 3}
        with torch.set_grad_enabled(train):
            a = render(inp["batch"], pkg, bg, crop_window=True)["render"]
            b = render(inp["batch"], pkg, bg, crop_window=False)["render"]
        assert tuple(a.shape) == (3, H, W) and torch.equal(a, b), float((a - b).abs().max())
        imgs.append(a.detach())
    assert torch.equal(imgs[0], imgs[1])


@pytest.mark.parametrize("k", [2, 3, 4])
def test_views_with_shared_geometry(k):
    """k cameras of one set of Gaussians (P = 209) in one pass: lists per view against the oracle, images against single renders."""
    from d3ga_amd import rasterizer as R
    from d3ga_amd import synthetic as syn
    from d3ga_amd.renderer import render, render_views
    P = 209
    inp = _scene(SEEDS[P])
    g = _gaussians(P)
    batches = [syn.make_batch(W, H, azimuth=0.4 + 0.7 * v) for v in range(k)]
    bg = torch.tensor([0.3, 0.6, 0.1])
    pkg = {"means3D": g["means3D"].to(DEV), "cov3D_precomp": g["cov6"].to(DEV), "opacities": g["opacities"].to(DEV),
           "shs": g["shs"].to(DEV), "rgb": None, "sh_degree": 3}
    for train in (False, True):
        pkg["means3D"] = g["means3D"].to(DEV).requires_grad_(train)
        with torch.set_grad_enabled(train):
            out = render_views(batches, pkg, bg.to(DEV))["render"].detach()
            binning, cap = R._last[torch.cuda.current_device()]
            start, plist, _ = R.tile_lists(binning, W, 16 * ((H + 15) // 16) * k, cap)
            start, plist = _np(start), _np(plist)
            singles = [render(batches[v], pkg, bg.to(DEV))["render"].detach() for v in range(k)]
        tiles = ((W + 15) // 16) * ((H + 15) // 16)
        base = 0
        for v in range(k):
            cam = oc.camera(batches[v]["R"], batches[v]["T"], batches[v]["FoVx"], batches[v]["FoVy"])
            ostart, olist, D, _, _ = _oracle(g, dict(inp, cam=cam), bg)
            np.testing.assert_array_equal(start[v * tiles:(v + 1) * tiles + 1] - base, ostart, err_msg=f"view {v}")
            np.testing.assert_array_equal(plist[base:base + D], olist + v * P, err_msg=f"view {v}")
            base += D
            assert torch.equal(out[v], singles[v]), (v, train)
        assert start[-1] == base and base > 0


@pytest.mark.parametrize("P", [1, 65, 209, 257])
def test_gradients_against_the_oracle(P):
    from d3ga_amd.rasterizer import GaussianRasterizer
    inp = dict(_scene(SEEDS[P]), **{k: v for k, v in _gaussians(P).items() if k != "P"})
    bg = torch.tensor([1.0, 0.5, 0.2])
    gpix = torch.randn(3, H, W, generator=torch.Generator().manual_seed(1))
    cu = lambda t: t.to(DEV).clone().contiguous().requires_grad_(True)
    means, cov, op, sh = (cu(inp[k]) for k in ("means3D", "cov6", "opacities", "shs"))
    m2d = torch.zeros_like(means, requires_grad=True)
    color, radii, _ = GaussianRasterizer(_settings(inp, bg, 3))(means3D=means, means2D=m2d, opacities=op, shs=sh, cov3D_precomp=cov)
    ocolor, oradii, _, ctx, og = _parity_oracle(inp, bg, gpix, 3)
    np.testing.assert_array_equal(_np(radii), oradii)
    par = Parity(ctx)
    assert par.gauss_share <= MAX_MARGINAL_GAUSSIANS, (P, SEEDS[P], par.gauss_share)
    (color * gpix.to(DEV)).sum().backward()
    _assert_grads(par, ((means.grad, og["means3D"], "means3D"), (cov.grad, og["cov3D"], "cov3D"), (op.grad, og["opacities"], "opacity"),
                        (sh.grad, og["shs"], "sh"), (m2d.grad, og["means2D"], "means2D")))


# ---------------------------------------------------------------------------------------------------------------------------------
# cage deformation, forward and backward
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("merged", [True, False], ids=["merge", "corners"])
@pytest.mark.parametrize("dbary", [False, True], ids=["plain", "delta_exp"])
@pytest.mark.parametrize("per_tet", [False, True], ids=["per_gaussian", "per_tet"])
@pytest.mark.parametrize("P", [1, 255, 257])
def test_cage_deform_against_the_oracle(P, per_tet, dbary, merged):
    """Values and every gradient against oracle/deform.py in float64, at the bars of test_gpu_parity.py::test_cage_deform_fuzz
    (means rtol 1e-4 / atol 1e-5, covariance 1e-4 relative, gradients element-wise 1e-3 |b| + 1e-6 max |b| -- 1e-5 for the vertex
    gradient, a long float32 sum -- plus four times what one float32 rounding of the inputs moves the element by).  dbary: with
    delta_barys and scale_activation="exp"."""
    from d3ga_amd import cage_deform as cd
    seed = 40 + P
    g = torch.Generator().manual_seed(seed)
    V, T = 60, 90
    canon = torch.randn(V, 3, generator=g)
    tetras = torch.stack([torch.randperm(V, generator=g)[:4] for _ in range(T)]).int()
    tet_id = torch.sort(torch.randint(0, T, (P,), generator=g)).values.int()
    barys = torch.rand(P, 4, generator=g); barys = barys / barys.sum(1, keepdim=True)
    # the canonical gradient in float64, rounded ONCE to float32: the (T,3,3) table, and the per-Gaussian layout as its rows -- the
    # oracle and both layouts of the product read the same float32 values
    table = od.canonical_gradient(canon.double(), tetras.long(), torch.arange(T))
    assert torch.isfinite(table).all() and float(table.abs().max()) < 1e4, "a degenerate tetrahedron: pick another seed"
    table = table.float()
    cg_g = table[tet_id.long()].contiguous()
    tp0 = canon + 0.1 * torch.randn(V, 3, generator=g)
    raw_s, rot, db = 0.3 * torch.randn(P, 3, generator=g) - 2.0, torch.randn(P, 4, generator=g), 0.05 * torch.randn(P, 4, generator=g)
    up_m, up_c = torch.randn(P, 3, generator=g), torch.randn(P, 6, generator=g)

    def oracle(eps, draw=0):
        ge = torch.Generator().manual_seed(seed + 77 + 1000 * draw)
        nz = lambda t: t.double() * (1.0 + eps * (2.0 * torch.rand(t.shape, generator=ge).double() - 1.0))
        tp64, b64, s64, r64, d64 = (nz(t).requires_grad_(True) for t in (tp0, barys, raw_s, rot, db))
        m64, c64 = od.cage_deform(tp64, tetras.long(), tet_id.long(), (b64 + d64) if dbary else b64, nz(cg_g), torch.exp(s64), r64)
        ((m64 * up_m.double()).sum() + (c64 * up_c.double()).sum()).backward()
        return m64, c64, tp64, b64, s64, r64, d64
    m64, c64, *leaves64 = oracle(0.0)
    moved = [oracle(6e-8, d)[2:] for d in range(4)]
    cu = lambda t: t.to(DEV).clone().contiguous().requires_grad_(True)
    tp, b, sr, r, d = (cu(t) for t in (tp0, barys, raw_s, rot, db))
    cg = (table if per_tet else cg_g).to(DEV)
    cd._merge_policy["enabled"] = merged
    try:
        if dbary:
            m, c = cd.cage_deform(tp, tetras.to(DEV), tet_id.to(DEV), b, cg, sr, r, delta_barys=d, scale_activation="exp")
        else:
            m, c = cd.cage_deform(tp, tetras.to(DEV), tet_id.to(DEV), b, cg, torch.exp(sr), r)
        ((m * up_m.to(DEV)).sum() + (c * up_c.to(DEV)).sum()).backward()
    finally:
        cd._merge_policy["enabled"] = True
    tag = (P, per_tet, dbary, merged)
    np.testing.assert_allclose(_np(m), m64.detach().numpy(), rtol=1e-4, atol=1e-5, err_msg=str(tag))
    assert rel_err(_np(c), c64.detach().numpy()) < 1e-4, tag
    pairs = [(tp.grad, 0, "tetpoints"), (b.grad, 1, "barys"), (sr.grad, 2, "scales"), (r.grad, 3, "rot")] + ([(d.grad, 4, "dbary")] if dbary else [])
    for mine, j, name in pairs:
        a, b_ = _np(mine).astype(np.float64), leaves64[j].grad.numpy()
        sens = np.max([np.abs(mv[j].grad.numpy() - b_) for mv in moved], axis=0)
        allow = 1e-3 * np.abs(b_) + (1e-5 if name == "tetpoints" else 1e-6) * np.abs(b_).max() + 4.0 * sens
        ex = float((np.abs(a - b_) / allow).max())
        assert ex <= 1.0, (tag, name, ex)
