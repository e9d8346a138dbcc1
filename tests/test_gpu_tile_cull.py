"""Tile lists from the alpha >= 1/255 box (d3ga_raster_params::tile_cull; d3ga_math.h: tile_rect_tight).  Claim under test: with the
rule on, preprocess lists a Gaussian only in the tiles of the reference's rectangle that its alpha >= 1/255 box reaches, and nothing
else changes -- the image, the radii and the visible count are the reference rule's bit for bit, every tile's list is a subsequence
of the reference rule's list in the same order, every dropped (tile, Gaussian) pair has alpha < 1/255 on all 256 pixels of the tile
(recomputed in float64 from the GPU's own records), and the gradients agree with the reference rule's within its own run-to-run
spread.  The rule is switched through GaussianRasterizationSettings.tile_cull (and, for the operators of renderer.py, through
rasterizer.set_tile_cull)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from util import scene_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ("means3D", "cov6", "opacities", "shs", "rgb")


def _np(t):
    return np.ascontiguousarray(t.detach().cpu().numpy())


@functools.lru_cache(maxsize=None)
def _scene(name, scale_mult, width=None, height=None):
    return scene_inputs(name, scale_mult=scale_mult, width=width, height=height)


def _take(inp, idx):
    g = {k: inp[k][idx].clone().contiguous() for k in KEYS}
    g["P"] = g["means3D"].shape[0]
    return g


def _settings(inp, bg, sh_degree, cull):
    from d3ga_amd.rasterizer import GaussianRasterizationSettings
    return GaussianRasterizationSettings(
        image_height=inp["H"], image_width=inp["W"], tanfovx=inp["cam"]["tanfovx"], tanfovy=inp["cam"]["tanfovy"], bg=bg.to(DEV),
        scale_modifier=1.0, viewmatrix=inp["view"].to(DEV), projmatrix=inp["proj"].to(DEV), sh_degree=sh_degree,
        campos=inp["campos"].to(DEV), prefiltered=False, debug=False, antialiasing=False, tile_cull=cull)


def _records(P):
    """(conic_o (P,4), xyh (P,4)) of the most recent single-view forward: the GPU's own per-Gaussian records (layout: csrc/
    d3ga_internal.h carve_geom -- sections of 4, 16, 16, 8, 1, 24, 16 bytes per Gaussian, each padded to 256 bytes)."""
    from d3ga_amd import rasterizer as R
    geom = R._last_img[torch.cuda.current_device()][3]
    a = lambda n: (n + 255) // 256 * 256
    off_conic = a(4 * P)
    off_xyh = off_conic + a(16 * P) + a(16 * P) + a(8 * P) + a(P) + a(24 * P)
    rec = lambda off: _np(geom[off:off + 16 * P].view(torch.float32).view(P, 4)).astype(np.float64)
    return rec(off_conic), rec(off_xyh)


def _render(g, inp, bg, cull, use_sh=True, train=False, gpix=None):
    """One render through the drop-in module with the rule on / off -> dict(image, radii, start, plist, cnt, conic_o, xyh[, grads])"""
    from d3ga_amd import rasterizer as R
    rast = R.GaussianRasterizer(_settings(inp, bg, 3 if use_sh else 0, cull))
    t = {k: g[k].to(DEV) for k in KEYS}
    leaves = ("means3D", "cov6", "opacities", "shs" if use_sh else "rgb")
    if train:
        for k in leaves:
            t[k].requires_grad_(True)
    with torch.set_grad_enabled(train):
        color, radii, _ = rast(means3D=t["means3D"], means2D=None, opacities=t["opacities"], shs=t["shs"] if use_sh else None,
                               colors_precomp=None if use_sh else t["rgb"], cov3D_precomp=t["cov6"])
    start, plist, _ = R.last_tile_lists(inp["W"], inp["H"])
    out = dict(image=color.detach(), radii=radii, start=_np(start), plist=_np(plist), cnt=R.last_counters())
    out["conic_o"], out["xyh"] = _records(g["P"]) if g["P"] else (np.zeros((0, 4)), np.zeros((0, 4)))
    if gpix is not None:
        (color * gpix).sum().backward()
        torch.cuda.synchronize()
        out["grads"] = {k: t[k].grad.clone() for k in leaves}
    return out


def _pairs(start, plist, stride):
    """the lists as one array of tile * stride + Gaussian, tile by tile in list order"""
    tile = np.repeat(np.arange(start.size - 1), np.diff(start))
    return tile.astype(np.int64) * stride + plist[:tile.size]


def _assert_same_render_from_shorter_lists(on, off, stride, what=""):
    """Everything the issue states for one on / off pair but the alpha test.  -> the dropped pairs (tile * stride + Gaussian)"""
    assert torch.equal(on["image"], off["image"]), (what, float((on["image"] - off["image"]).abs().max()))
    assert torch.equal(on["radii"], off["radii"]), what
    assert on["cnt"]["visible"] == off["cnt"]["visible"], (what, on["cnt"], off["cnt"])
    assert not on["cnt"]["overflow"] and not off["cnt"]["overflow"], what
    assert on["cnt"]["D"] <= off["cnt"]["D"] and on["cnt"]["max_tile"] <= off["cnt"]["max_tile"], (what, on["cnt"], off["cnt"])
    assert on["cnt"]["D"] == int(on["start"][-1]) and off["cnt"]["D"] == int(off["start"][-1]), what
    p_on, p_off = _pairs(on["start"], on["plist"], stride), _pairs(off["start"], off["plist"], stride)
    assert np.unique(p_off).size == p_off.size
    keep = np.isin(p_off, p_on)
    # a subsequence in the same order: what is left of the reference rule's lists after dropping IS the tight rule's lists
    assert int(keep.sum()) == p_on.size, (what, int(keep.sum()), p_on.size)
    np.testing.assert_array_equal(p_off[keep], p_on, err_msg=f"order of the shortened lists {what}")
    return p_off[~keep]


def _assert_dropped_pairs_reach_no_pixel(dropped, stride, rec, W, what=""):
    """alpha of every dropped (tile, Gaussian) on the tile's 256 pixels, float64 from the GPU's conic_o / xyh records (the forward's
    rule: a pixel blends the entry when power <= 0 and min(0.99, opacity exp(power)) >= 1/255)"""
    if dropped.size == 0:
        return 0.0
    conic_o, xyh = rec
    gx = (W + 15) // 16
    tile, gid = dropped // stride, dropped % stride
    x0, y0 = 16.0 * (tile % gx), 16.0 * (tile // gx)
    px = x0[:, None, None] + np.arange(16.0)[None, None, :]
    py = y0[:, None, None] + np.arange(16.0)[None, :, None]
    a, b, c, o = (conic_o[gid, j][:, None, None] for j in range(4))
    dx, dy = xyh[gid, 0][:, None, None] - px, xyh[gid, 1][:, None, None] - py
    power = -0.5 * (a * dx * dx + c * dy * dy) - b * dx * dy
    alpha = np.where(power <= 0.0, o * np.exp(np.minimum(power, 0.0)), 0.0)
    worst = float(alpha.max())
    assert worst < 1.0 / 255.0, (what, worst, int(gid[np.argmax(alpha.reshape(alpha.shape[0], -1).max(1))]))
    return worst


# T1 at scale x1 and x3; P = 1, 63, 64, 65: a partial, a nearly full, a full wavefront and one Gaussian into the second; 257: one
# into the second block; 577 = 64 x 9 + 1: a last wavefront of one Gaussian in a third block -- every fifth Gaussian, so that P of
# them still span the body.  SH and precomputed colours, inference and training forward: the four kernel variants.
@pytest.mark.parametrize("scale_mult", [1.0, 3.0])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 257, 577])
def test_shapes_and_kernel_variants(P, scale_mult):
    inp = _scene("T1", scale_mult)
    g = _take(inp, torch.arange(P) * 5)
    bg = torch.tensor([0.2, 0.4, 0.6])
    for use_sh in (True, False):
        for train in (False, True):
            what = f"P={P} x{scale_mult} sh={use_sh} train={train}"
            off = _render(g, inp, bg, False, use_sh, train)
            on = _render(g, inp, bg, True, use_sh, train)
            assert off["cnt"]["D"] > 0
            dropped = _assert_same_render_from_shorter_lists(on, off, P, what)
            # every other record the forward reads is the same bit for bit
            np.testing.assert_array_equal(on["conic_o"], off["conic_o"]); np.testing.assert_array_equal(on["xyh"], off["xyh"])
            worst = _assert_dropped_pairs_reach_no_pixel(dropped, P, (off["conic_o"], off["xyh"]), inp["W"], what)
            print(f"{what}: D {off['cnt']['D']} -> {on['cnt']['D']}, max_tile {off['cnt']['max_tile']} -> {on['cnt']['max_tile']}, "
                  f"largest alpha x 255 of a dropped pair {255 * worst:.4f}")


def test_tightness_and_conservativeness_on_the_whole_scene():
    """T1 x1, all 3000 Gaussians: at most 0.90 of the reference rule's duplicates are left (a CPU count of the same rule on the
    flagship scene's views gives 0.81-0.85), and none of the dropped pairs reaches a pixel."""
    inp = _scene("T1", 1.0)
    g = _take(inp, torch.arange(inp["means3D"].shape[0]))
    assert g["P"] == 3000
    bg = torch.tensor([0.3, 0.6, 0.1])
    off, on = _render(g, inp, bg, False), _render(g, inp, bg, True)
    dropped = _assert_same_render_from_shorter_lists(on, off, g["P"])
    worst = _assert_dropped_pairs_reach_no_pixel(dropped, g["P"], (off["conic_o"], off["xyh"]), inp["W"])
    ratio = on["cnt"]["D"] / off["cnt"]["D"]
    print(f"T1 x1: D {off['cnt']['D']} -> {on['cnt']['D']} ({ratio:.3f}), max_tile {off['cnt']['max_tile']} -> {on['cnt']['max_tile']}, "
          f"largest alpha x 255 of a dropped pair {255 * worst:.4f}")
    assert on["cnt"]["D"] <= 0.90 * off["cnt"]["D"], ratio


@pytest.mark.parametrize("use_sh", [True, False])
def test_gradients_of_a_random_image_loss(use_sh):
    """On against off, per tensor in the max-norm: within 8 x the off path's own run-to-run spread (the compositing backward sums
    with float atomics; the bar of docs/LOG.md "Deform backward as the tail") -- which is bit equality wherever the off path
    repeats itself bit for bit, dL/dSH and dL/dopacity included."""
    inp = _scene("T1", 3.0)
    g = _take(inp, torch.arange(inp["means3D"].shape[0]))
    bg = torch.tensor([0.3, 0.6, 0.1])
    gpix = torch.randn(3, inp["H"], inp["W"], generator=torch.Generator().manual_seed(5)).to(DEV)
    offs = [_render(g, inp, bg, False, use_sh, True, gpix)["grads"] for _ in range(3)]
    on = _render(g, inp, bg, True, use_sh, True, gpix)["grads"]
    for k in on:
        spread = max(float((offs[i][k] - offs[j][k]).abs().max()) for i in range(3) for j in range(i))
        diff = float((on[k] - offs[0][k]).abs().max())
        scale = float(offs[0][k].abs().max())
        print(f"dL/d{k}: max |on - off| {diff:.3e}, off run-to-run spread {spread:.3e}, max |off| {scale:.3e}")
        assert scale > 0
        assert diff <= 8.0 * spread, (k, diff, spread)


def test_a_gaussian_below_one_255th_stays_visible_in_one_tile():
    inp = _scene("T1", 3.0)
    g = _take(inp, torch.arange(600) * 5)
    faint = [7, 130, 333]
    g["opacities"][faint] = 0.003                                # x 255 < 1: no pixel can blend it (hx = -1)
    bg = torch.tensor([0.5, 0.5, 0.0])
    off, on = _render(g, inp, bg, False), _render(g, inp, bg, True)
    _assert_same_render_from_shorter_lists(on, off, g["P"], "faint")
    for i in faint:
        assert int(off["radii"][i]) > 0 and int(on["radii"][i]) > 0
        assert float(on["xyh"][i, 2]) == -1.0
        n_off, n_on = int((off["plist"] == i).sum()), int((on["plist"] == i).sum())
        assert n_off >= 1 and n_on == 1, (i, n_off, n_on)


def test_screen_filling_splats_take_the_unreserved_path():
    """512 x 320 = 640 tiles, more than a reservation record holds: the wavefronts of the two screen-filling splats go unreserved
    (tests/test_gpu_binning_reserve.py: test_windows_larger_than_a_record) under both rules -- their alpha boxes fill the screen too."""
    inp = _scene("T1", 3.0, 512, 320)
    g = _take(inp, torch.arange(5 * 64 + 3) * 3)
    for i in (70, 200):
        g["cov6"][i] = torch.tensor([4.0, 0.0, 0.0, 4.0, 0.0, 4.0])
        g["opacities"][i] = 0.05
    bg = torch.tensor([0.1, 0.2, 0.3])
    for train in (False, True):
        off, on = _render(g, inp, bg, False, True, train), _render(g, inp, bg, True, True, train)
        dropped = _assert_same_render_from_shorter_lists(on, off, g["P"], f"huge train={train}")
        _assert_dropped_pairs_reach_no_pixel(dropped, g["P"], (off["conic_o"], off["xyh"]), inp["W"], "huge")
        for i in (70, 200):
            assert int((off["plist"] == i).sum()) == 640 and int((on["plist"] == i).sum()) == 640
        assert on["cnt"]["D"] < off["cnt"]["D"]


def test_all_culled():
    inp = _scene("T1", 3.0)
    g = _take(inp, torch.arange(300))
    g["means3D"][:, 2] -= 100.0                                  # behind the camera (azimuth 0.4)
    bg = torch.tensor([0.7, 0.1, 0.3])
    off, on = _render(g, inp, bg, False), _render(g, inp, bg, True)
    _assert_same_render_from_shorter_lists(on, off, g["P"], "all culled")
    assert on["cnt"]["D"] == 0 and on["cnt"]["visible"] == 0 and int(on["radii"].max()) == 0
    assert torch.equal(on["image"], bg.to(DEV)[:, None, None].expand_as(on["image"]))


def _override(mode):
    from d3ga_amd import rasterizer as R

    class _Ctx:
        def __enter__(self):
            R.set_tile_cull(mode)

        def __exit__(self, *exc):
            R.set_tile_cull(None)
            return False
    return _Ctx()


def _pkg(g, train=False):
    return {"means3D": g["means3D"].to(DEV).requires_grad_(train), "cov3D_precomp": g["cov6"].to(DEV), "opacities": g["opacities"].to(DEV),
            "shs": g["shs"].to(DEV), "rgb": None, "sh_degree": 3}


def test_windowed_camera_slot():
    """The rectangle is tightened on the view's full raster and clipped to the window afterwards: the window render under either rule
    is the padded render pasted, bit for bit, from fewer duplicates."""
    from d3ga_amd import rasterizer as R
    from d3ga_amd.renderer import render
    W, H, cx, cy = 161, 143, 57, 96
    inp = scene_inputs("T1", scale_mult=3.0, cx=cx, cy=cy, width=W, height=H)
    g = _take(inp, torch.arange(1000) * 3)
    bg = torch.tensor([0.3, 0.6, 0.1], device=DEV)
    for train in (False, True):
        res = {}
        for cull in (False, True):
            with _override(cull), torch.set_grad_enabled(train):
                a = render(inp["batch"], _pkg(g, train), bg, crop_window=True)["render"]
                cnt = R.last_counters()
                b = render(inp["batch"], _pkg(g, train), bg, crop_window=False)["render"]
            assert tuple(a.shape) == (3, H, W) and torch.equal(a, b)
            res[cull] = (a.detach(), cnt)
        assert torch.equal(res[True][0], res[False][0])
        assert not res[True][1]["overflow"] and res[True][1]["visible"] == res[False][1]["visible"]
        assert 0 < res[True][1]["D"] < res[False][1]["D"], (res[True][1], res[False][1])


def _batched_lists(W, H, k):
    from d3ga_amd import rasterizer as R
    binning, cap = R._last[torch.cuda.current_device()]
    start, plist, _ = R.tile_lists(binning, W, 16 * ((H + 15) // 16) * k, cap)
    return _np(start), _np(plist)


def test_render_views_with_two_cameras():
    from d3ga_amd import rasterizer as R
    from d3ga_amd import synthetic as syn
    from d3ga_amd.renderer import render, render_views
    inp = _scene("T1", 3.0)
    W, H, k = inp["W"], inp["H"], 2
    g = _take(inp, torch.arange(900) * 3 + 1)
    batches = [syn.make_batch(W, H, azimuth=0.4), syn.make_batch(W, H, azimuth=2.5, fill=1.0)]
    bg = torch.tensor([0.3, 0.6, 0.1], device=DEV)
    res = {}
    with torch.no_grad():
        for cull in (False, True):
            out = render_views(batches, _pkg(g), bg, tile_cull=cull)["render"]
            start, plist = _batched_lists(W, H, k)
            res[cull] = dict(image=out, radii=torch.zeros(0), start=start, plist=plist, cnt=R.last_counters())
        singles = [render(b, _pkg(g), bg)["render"] for b in batches]       # (render: the rule is on)
    res[True]["radii"] = res[False]["radii"]
    dropped = _assert_same_render_from_shorter_lists(res[True], res[False], k * g["P"], "k = 2")
    assert dropped.size > 0
    for v in range(k):
        assert torch.equal(res[True]["image"][v], singles[v]), v
    # gradients of the batch under the rule: the sum over the views, as without it
    grads = {}
    for cull in (False, True):
        pkg = _pkg(g, True)
        render_views(batches, pkg, bg, tile_cull=cull)["render"].square().mean().backward()
        grads[cull] = pkg["means3D"].grad.clone()
    scale = float(grads[False].abs().max())
    assert scale > 0 and float((grads[True] - grads[False]).abs().max()) <= 1e-4 * scale      # float atomics: order-dependent rounding


def test_render_pair_and_geometry_reuse():
    from d3ga_amd import rasterizer as R
    from d3ga_amd.renderer import render, render_pair
    inp = _scene("T1", 3.0)
    g = _take(inp, torch.arange(1200) * 2)
    bg, bg0 = torch.tensor([0.3, 0.6, 0.1], device=DEV), torch.zeros(3, device=DEV)
    sil = torch.rand(g["P"], 3, generator=torch.Generator().manual_seed(4)).to(DEV)
    res = {}
    for cull in (False, True):
        with _override(cull), torch.no_grad():
            out = render_pair(inp["batch"], _pkg(g), bg, sil, bg0)
            res[cull] = (out["render"], out["render2"], R.last_counters())
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])
    assert 0 < res[True][2]["D"] < res[False][2]["D"] and res[True][2]["visible"] == res[False][2]["visible"]
    # render() asks for the tight rule by itself; geometry_reuse(): the silhouette pass shares the first pass's (tight) binning, and
    # a pass under the other rule must not -- the rule is part of the cache key
    pkg = _pkg(g)
    with torch.no_grad(), R.geometry_reuse():
        a = render(inp["batch"], pkg, bg)["render"]
        d_first = R.last_counters()["D"]
        b = render(inp["batch"], pkg, bg0, colors_precomp=sil)["render"]
        assert R.last_counters()["D"] == d_first == res[True][2]["D"]
        with _override(False):
            c = render(inp["batch"], pkg, bg0, colors_precomp=sil)["render"]
            assert R.last_counters()["D"] == res[False][2]["D"]
    assert torch.equal(a, res[True][0]) and torch.equal(b, res[True][1]) and torch.equal(c, b)


def test_captured_step_replayed_with_two_cameras_under_a_capacity_sized_from_the_tight_lists():
    """One captured training step (render_l1 behind the cage deformation) replayed with two cameras equals eager; the static
    capacity holds the tight rule's duplicates of either camera and not the reference rule's."""
    from d3ga_amd import rasterizer as R
    from d3ga_amd import synthetic as syn
    from d3ga_amd.cage_deform import cage_deform
    from d3ga_amd.cameras import CameraSlot
    from d3ga_amd.graph import CapturedStep
    from d3ga_amd.renderer import render_l1
    inp = _scene("T1", 3.0)
    sc = inp["scene"]
    W, H = inp["W"], inp["H"]
    leaf = lambda t: t.to(DEV).clone().contiguous().requires_grad_(True)
    tp, sh, lg = leaf(inp["tetpoints"]), leaf(inp["shs"]), leaf(torch.logit(inp["opacities"].clamp(1e-4, 1 - 1e-4)))
    consts = [sc["tetras"].to(DEV), sc["tetra_id"].to(DEV), sc["barys"].to(DEV), inp["canon_grad"].to(DEV), inp["scales"].to(DEV),
              sc["rotation"].to(DEV)]
    bg = torch.ones(3, device=DEV)
    cams = [syn.make_batch(W, H, azimuth=0.4), syn.make_batch(W, H, azimuth=1.7)]
    targets = [torch.rand(3, H, W, generator=torch.Generator().manual_seed(60 + v)).to(DEV) for v in range(2)]
    params = (tp, sh, lg)

    def step(batch, target):
        means, cov6 = cage_deform(tp, *consts)
        out = render_l1(batch, {"means3D": means, "cov3D_precomp": cov6, "opacity_logits": lg, "shs": sh, "rgb": None, "sh_degree": 3}, bg, target)
        out["l1"].backward()
        return out["render"].detach(), out["l1"].detach()

    eager, d_on, d_off = [], 0, 0
    for b, t in zip(cams, targets):
        with _override(False):
            step(b, t)
            d_off = max(d_off, R.last_counters()["D"])
        for p in params:
            p.grad = None
        img, loss = step(b, t)
        start, plist, _ = R.last_tile_lists(W, H)
        eager.append((img.clone(), float(loss), [p.grad.clone() for p in params], _np(start), _np(plist)))
        d_on = max(d_on, R.last_counters()["D"])
    cap = d_on + 32
    assert cap < d_off, (d_on, d_off)
    R.set_capacity_policy("static", cap)
    try:
        slot = CameraSlot(W, H, device=DEV).set(cams[0])
        target = targets[0].clone()
        slot_batch = dict(cams[0], camera_slot=slot)
        for p in params:
            p.grad = None
        graph = CapturedStep(lambda: step(slot_batch, target), params=params, slots={"target": target}, camera=slot)
        for v in (1, 0, 1):
            img_g, loss_g = graph.replay(camera=cams[v], target=targets[v])
            torch.cuda.synchronize()
            cnt = R.last_counters()
            img_e, loss_e, grads_e, start_e, plist_e = eager[v]
            assert not cnt["overflow"] and cnt["D"] == int(start_e[-1]) <= cap
            start, plist, _ = R.last_tile_lists(W, H)
            np.testing.assert_array_equal(_np(start), start_e)
            np.testing.assert_array_equal(_np(plist), plist_e)
            assert torch.equal(img_g, img_e), v
            assert abs(float(loss_g) - loss_e) <= 1e-6 * abs(loss_e) + 1e-9
            for p, ge in zip(params, grads_e):
                scale = float(ge.abs().max())
                assert float((p.grad - ge).abs().max()) <= 1e-4 * scale, v      # float atomics: order-dependent rounding
    finally:
        R.set_capacity_policy("auto")
