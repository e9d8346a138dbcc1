"""Binning with slots reserved in preprocess (d3ga_amd/csrc/d3ga_internal.h: reservation records).  Every wavefront of the
preprocess kernels counts its duplicates in a tile window of its own, reserves their slots with one returning atomic per tile and
leaves box and bases in its record; the scatter pass places the keys from the record.  Claim under test: the tile offsets and the
depth-sorted lists are those of the C oracle BIT FOR BIT (integer work: no tolerance), the counters are the oracle's, and images
are bit-identical to a render of the same Gaussians laid out one per wavefront -- at the Gaussian counts where the last wavefront
and the last block are partial, with whole wavefronts culled, through the unreserved path of windows larger than a record, at a
capacity below the duplicate count, over a binning scratch full of garbage, view-batched, windowed and under graph replay."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from oracle import camera as oc
from oracle import raster_c as rc
from util import scene_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
RECORD_TILES = 508          # window tiles a reservation record holds (kResvTiles)
KEYS = ("means3D", "cov6", "opacities", "shs", "rgb")


def _np(t):
    return np.ascontiguousarray(t.detach().cpu().numpy())


@functools.lru_cache(maxsize=None)
def _scene(name, scale_mult, width=None, height=None):
    return scene_inputs(name, scale_mult=scale_mult, width=width, height=height)


def _take(inp, idx):
    """The Gaussians `idx` of a scene, as a set of inputs of their own."""
    g = {k: inp[k][idx].clone().contiguous() for k in KEYS}
    g["P"] = g["means3D"].shape[0]
    return g


def _cull(g, mask):
    """Move the Gaussians `mask` behind the camera (every scene here is seen from azimuth 0.4: 100 m along -z is behind it)."""
    g = dict(g)
    m = g["means3D"].clone()
    m[mask, 2] -= 100.0
    g["means3D"] = m
    return g


def _spread(g):
    """One Gaussian per wavefront: Gaussian i at index 64 i, the other 63 of its wavefront culled copies.  The index order is kept,
    so every tile list holds the same Gaussians in the same order and the image must not change in a single bit."""
    P = g["P"]
    idx = torch.arange(64 * P) // 64
    s = _take(g, idx)
    keep = torch.zeros(64 * P, dtype=torch.bool)
    keep[::64] = True
    return _cull(s, ~keep)


def _settings(inp, bg, sh_degree):
    from d3ga_amd.rasterizer import GaussianRasterizationSettings
    return GaussianRasterizationSettings(
        image_height=inp["H"], image_width=inp["W"], tanfovx=inp["cam"]["tanfovx"], tanfovy=inp["cam"]["tanfovy"], bg=bg.to(DEV),
        scale_modifier=1.0, viewmatrix=inp["view"].to(DEV), projmatrix=inp["proj"].to(DEV), sh_degree=sh_degree,
        campos=inp["campos"].to(DEV), prefiltered=False, debug=False, antialiasing=False)


def _render(g, inp, bg, use_sh=True, train=False):
    """-> (image, radii, tile_start, point_list, counters).  train: a backward may follow, so the forward is the one that leaves
    d(colour)/d(direction) (the flagship's kernel variant); else the inference variant."""
    from d3ga_amd import rasterizer as R
    rast = R.GaussianRasterizer(_settings(inp, bg, 3 if use_sh else 0))
    t = {k: g[k].to(DEV) for k in KEYS}
    if train:
        t["means3D"].requires_grad_(True)
    with torch.set_grad_enabled(train):
        color, radii, _ = rast(means3D=t["means3D"], means2D=None, opacities=t["opacities"], shs=t["shs"] if use_sh else None,
                               colors_precomp=None if use_sh else t["rgb"], cov3D_precomp=t["cov6"])
    start, plist, _ = R.last_tile_lists(inp["W"], inp["H"])
    return color.detach(), radii, start, plist, R.last_counters()


def _oracle(g, inp, bg, use_sh=True):
    """-> (tile_start, point_list, D, visible) of the C oracle"""
    cam = inp["cam"]
    kw = dict(shs=_np(g["shs"]), sh_degree=3) if use_sh else dict(colors_precomp=_np(g["rgb"]))
    _, radii, _, ctx = rc.forward(_np(g["means3D"]), _np(g["opacities"]), _np(bg), cam["world_view_transform"], cam["full_proj_transform"],
                                  cam["camera_center"], cam["tanfovx"], cam["tanfovy"], inp["W"], inp["H"], cov3D_precomp=_np(g["cov6"]), **kw)
    ostart, olist = rc.tile_lists(ctx)
    return np.asarray(ostart), np.asarray(olist), rc.num_rendered(ctx), int((radii > 0).sum())


def _assert_lists(out, ref, what=""):
    _, _, start, plist, cnt = out
    ostart, olist, D, visible = ref
    np.testing.assert_array_equal(_np(start), ostart, err_msg=f"tile offsets {what}")
    np.testing.assert_array_equal(_np(plist), olist, err_msg=f"sorted lists {what}")
    assert (cnt["D"], cnt["overflow"], cnt["visible"]) == (D, False, visible), (what, cnt)
    lengths = np.diff(ostart)
    assert cnt["max_tile"] == (int(lengths.max()) if lengths.size else 0), (what, cnt)


# P = 1, 63, 64, 65: a partial, a nearly full, a full wavefront and one Gaussian into the second; 255, 257: the same around a block;
# 64 k + 1 (k = 9): a last wavefront of one Gaussian in a third block.  The last two also through the kernel variants of a
# training forward and of precomputed colours (no SH slab: the window has LDS of its own).
@pytest.mark.parametrize("P,use_sh,train", [(1, True, False), (63, True, False), (64, True, True), (65, True, False), (255, True, True),
                                             (257, True, False), (577, True, True), (257, False, False), (577, False, True)])
def test_gaussian_counts(P, use_sh, train):
    inp = _scene("T1", 3.0)
    # every fifth Gaussian of the scene: neighbours in index are neighbours in space, and P of them still span the body
    g = _take(inp, torch.arange(P) * 5)
    bg = torch.tensor([0.2, 0.4, 0.6])
    out = _render(g, inp, bg, use_sh, train)
    ref = _oracle(g, inp, bg, use_sh)
    assert ref[2] > 0
    _assert_lists(out, ref, f"P={P}")
    if P <= 257:
        one = _render(_spread(g), inp, bg, use_sh, train)
        assert one[4]["D"] == ref[2] and torch.equal(one[0], out[0]), float((one[0] - out[0]).abs().max())
        np.testing.assert_array_equal(_np(one[3]), 64 * ref[1])


@pytest.mark.parametrize("pattern", ["culled_wavefronts", "all_culled", "one_tile"])
def test_culling_patterns(pattern):
    inp = _scene("T1", 3.0)
    bg = torch.tensor([0.7, 0.1, 0.3])
    if pattern == "culled_wavefronts":                       # wavefronts 1, 2 and 4 of 6 hold nothing visible, wavefront 5 is partial
        g = _take(inp, torch.arange(5 * 64 + 17) * 7)
        wave = torch.arange(g["P"]) // 64
        g = _cull(g, (wave == 1) | (wave == 2) | (wave == 4))
    elif pattern == "all_culled":
        g = _take(inp, torch.arange(300))
        g = _cull(g, torch.ones(300, dtype=torch.bool))
    else:                                                    # 200 small splats around one point: all duplicates in ONE tile
        g = _take(inp, torch.arange(200))
        c = inp["means3D"][2500]                           # (projects well inside a tile)
        g["means3D"] = (c.unsqueeze(0) + 1e-3 * torch.randn(200, 3, generator=torch.Generator().manual_seed(2))).contiguous()
        g["cov6"] = torch.tensor([1e-6, 0.0, 0.0, 1e-6, 0.0, 1e-6]).repeat(200, 1).contiguous()
    out = _render(g, inp, bg)
    ref = _oracle(g, inp, bg)
    _assert_lists(out, ref, pattern)
    if pattern == "all_culled":
        assert ref[2] == 0 and torch.equal(out[0], bg.to(DEV)[:, None, None].expand_as(out[0]))
    elif pattern == "one_tile":
        assert int((np.diff(ref[0]) > 0).sum()) == 1 and ref[2] == 200
    else:
        assert 0 < ref[3] <= 3 * 64 + 17 and int(_np(out[1])[64:192].max()) == 0 and int(_np(out[1])[256:320].max()) == 0
        one = _render(_spread(g), inp, bg)
        assert torch.equal(one[0], out[0])


@pytest.mark.parametrize("huge", [(70,), (70, 200), (70, 100, 200)])
def test_windows_larger_than_a_record(huge):
    """512 x 320: 640 tiles, more than a record holds.  A screen-filling splat makes its wavefront's window the whole grid, so that
    wavefront (small splats included) goes unreserved while the others reserve: every tile they touch holds reserved and unreserved
    duplicates together.  (70, 200): two unreserved wavefronts (1 and 3) share every tile; (70, 100, 200): two huge splats in one."""
    inp = _scene("T1", 3.0, 512, 320)
    tiles = 32 * 20
    assert tiles > RECORD_TILES
    g = _take(inp, torch.arange(5 * 64 + 3) * 3)
    for i in huge:
        g["cov6"][i] = torch.tensor([4.0, 0.0, 0.0, 4.0, 0.0, 4.0])
        g["opacities"][i] = 0.05
    bg = torch.tensor([0.1, 0.2, 0.3])
    ref = _oracle(g, inp, bg)
    for i in huge:
        assert int((ref[1] == i).sum()) == tiles, "the splat does not fill the screen"
    lengths = np.diff(ref[0])
    assert int((lengths > len(huge)).sum()) > 20, "no tile mixes the two kinds of duplicates"
    for train in (False, True):
        _assert_lists(_render(g, inp, bg, True, train), ref, f"huge={huge} train={train}")


def _filled_scratch(monkeypatch, byte, tail=0):
    """Every scratch buffer of the renders that follow starts out filled with `byte`, with `tail` more bytes of it behind the binning
    buffer; -> the list of binning buffers handed out (tail included)."""
    from d3ga_amd import rasterizer as R
    made = []
    plain = R._scratch

    def scratch(*a, **kw):
        bufs = plain(*a, **kw)
        if bufs[1] is not None:
            n = bufs[1].numel()
            big = torch.empty(n + tail, dtype=torch.uint8, device=bufs[1].device)
            big.fill_(byte)
            bufs[1] = big[:n]
            made.append(big)
        return bufs
    monkeypatch.setattr(R, "_scratch", scratch)
    return made


def test_static_capacity_below_the_duplicate_count(monkeypatch):
    """Overflow flag set, every list that ends below the capacity complete and sorted, the one across it a subset of the oracle's,
    and not a byte written behind `capacity` keys or list entries.  Guards: the padding behind both arrays up to their next 256-byte
    section (the capacity is chosen so that this is 128 and 64 bytes: 16 keys, 16 entries) and 64 KiB behind the whole buffer."""
    from d3ga_amd import _lib
    from d3ga_amd import rasterizer as R
    inp = _scene("T1", 4.0)
    g = _take(inp, torch.arange(3000))
    bg = torch.zeros(3)
    ostart, olist, D, visible = _oracle(g, inp, bg)
    cap = (D // 2) // 32 * 32 + 16                           # 8 cap = 128 and 4 cap = 192 modulo 256
    made = _filled_scratch(monkeypatch, 0xA5, tail=1 << 16)
    R.set_capacity_policy("static", cap)
    try:
        _, _, start, plist, cnt = _render(g, inp, bg)
    finally:
        R.set_capacity_policy("auto")
    assert cnt["overflow"] and cnt["D"] == D and cnt["visible"] == visible
    np.testing.assert_array_equal(_np(start), ostart)
    plist = _np(plist)
    assert plist.shape[0] == cap
    last = int(np.searchsorted(ostart, cap, side="right")) - 1            # the tile whose list crosses the capacity
    np.testing.assert_array_equal(plist[:ostart[last]], olist[:ostart[last]])
    assert set(plist[ostart[last]:cap].tolist()) <= set(olist[ostart[last]:ostart[last + 1]].tolist())
    off = (ctypes.c_int64 * 6)()
    assert _lib.lib().d3ga_raster_binning_layout(inp["W"], inp["H"], cap, off) == 0
    binning = made[-1]
    guard_keys = binning[off[4] + 8 * cap:off[5]]
    guard_list = binning[off[5] + 4 * cap:off[5] + ((4 * cap + 255) // 256) * 256]
    assert guard_keys.numel() == 128 and guard_list.numel() == 64
    assert bool((guard_keys == 0xA5).all()) and bool((guard_list == 0xA5).all())
    assert bool((binning[-(1 << 16):] == 0xA5).all())


@pytest.mark.parametrize("huge", [False, True])
def test_garbage_in_the_binning_scratch(monkeypatch, huge):
    """Records, counters and cursors of an earlier frame (here: 0xFF everywhere, then zeros) must not reach the lists."""
    W, H = (512, 320) if huge else (None, None)
    inp = _scene("T1", 3.0, W, H)
    g = _take(inp, torch.arange(700) * 4)
    g = _cull(g, (torch.arange(700) // 64) == 3)
    if huge:
        g["cov6"][400] = torch.tensor([4.0, 0.0, 0.0, 4.0, 0.0, 4.0])
    bg = torch.tensor([0.5, 0.5, 0.0])
    ref = _oracle(g, inp, bg)
    outs = []
    for byte in (0xFF, 0x00):
        made = _filled_scratch(monkeypatch, byte)
        outs.append(_render(g, inp, bg))
        assert len(made) >= 1
        monkeypatch.undo()
        _assert_lists(outs[-1], ref, f"fill {byte:#x}")
    assert torch.equal(outs[0][0], outs[1][0])


def _culling_batch(b):
    """The camera of `b` pushed 100 m forward along its axis: everything is behind it."""
    c = dict(b)
    c["T"] = np.asarray(b["T"], np.float64) + np.array([0.0, 0.0, -100.0])
    return c


def _batched_lists(W, H, k):
    """(tile_start, point_list) of the most recent forward, a batch of k views: one frame of k x tile rows (d3ga.h: n_views)"""
    from d3ga_amd import rasterizer as R
    binning, cap = R._last[torch.cuda.current_device()]
    start, plist, _ = R.tile_lists(binning, W, 16 * ((H + 15) // 16) * k, cap)
    return _np(start), _np(plist)


@pytest.mark.parametrize("frames", [False, True])
def test_view_batched(frames):
    """k = 3 with a camera that culls everything in the middle; frames: a batch of frames (every view its own geometry).  Lists
    against the oracle per view (record v P + i of the batch), images against the single-view renders."""
    from d3ga_amd import synthetic as syn
    from d3ga_amd.renderer import render, render_views
    inp = _scene("T1", 3.0)
    W, H, k = inp["W"], inp["H"], 3
    g = _take(inp, torch.arange(900) * 3 + 1)
    P = g["P"]
    batches = [syn.make_batch(W, H, azimuth=0.4), _culling_batch(syn.make_batch(W, H, azimuth=0.4)), syn.make_batch(W, H, azimuth=2.5, fill=1.0)]
    bg = torch.tensor([0.3, 0.6, 0.1])
    gen = torch.Generator().manual_seed(8)
    geo = [g if not frames or v == 0 else dict(g, means3D=g["means3D"] + 0.02 * torch.randn(P, 3, generator=gen)) for v in range(k)]
    pkgs = [{"means3D": geo[v]["means3D"].to(DEV), "cov3D_precomp": g["cov6"].to(DEV), "opacities": g["opacities"].to(DEV),
             "shs": g["shs"].to(DEV), "rgb": None, "sh_degree": 3} for v in range(k)]
    for p in pkgs[1:]:
        p["opacities"], p["shs"], p["cov3D_precomp"] = pkgs[0]["opacities"], pkgs[0]["shs"], pkgs[0]["cov3D_precomp"]
    with torch.no_grad():
        out = render_views(batches, pkgs if frames else pkgs[0], bg.to(DEV))["render"]
        start, plist = _batched_lists(W, H, k)
        singles = [render(batches[v], pkgs[v], bg.to(DEV))["render"] for v in range(k)]
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    base = 0
    for v in range(k):
        cam = oc.camera(batches[v]["R"], batches[v]["T"], batches[v]["FoVx"], batches[v]["FoVy"])
        ostart, olist, D, _ = _oracle(geo[v], dict(inp, cam=cam), bg)
        assert (D == 0) == (v == 1)
        np.testing.assert_array_equal(start[v * tiles:(v + 1) * tiles + 1] - base, ostart, err_msg=f"view {v}")
        np.testing.assert_array_equal(plist[base:base + D], olist + v * P, err_msg=f"view {v}")
        base += D
        assert torch.equal(out[v], singles[v]), v
    assert start[-1] == base


def test_window_that_cuts_the_wavefronts_boxes():
    """A windowed camera slot: the rectangles are clipped to the window before the wavefront forms its box, and Gaussians that miss
    the window leave their wavefront's reservation.  The window render is the padded render pasted, bit for bit."""
    from d3ga_amd.renderer import paste, render
    W, H, cx, cy = 161, 143, 57, 96                          # the window is the right / top part of a 208 x 192 raster
    inp = scene_inputs("T1", scale_mult=3.0, cx=cx, cy=cy, width=W, height=H)
    g = _take(inp, torch.arange(1000) * 3)
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
    assert torch.equal(imgs[0], imgs[1]) and float((imgs[0] - bg.view(3, 1, 1)).abs().max()) > 0.05


def test_captured_step_with_a_camera_that_empties_wavefronts():
    """One captured step replayed with two cameras equals eager.  Camera B is zoomed far in: whole wavefronts that reserved
    slots under camera A see nothing under B (and back), on the same binning scratch."""
    from d3ga_amd import rasterizer as R
    from d3ga_amd import synthetic as syn
    from d3ga_amd.cage_deform import cage_deform
    from d3ga_amd.cameras import CameraSlot
    from d3ga_amd.graph import CapturedStep
    from d3ga_amd.losses import l1_loss
    from d3ga_amd.renderer import render
    inp = _scene("T1", 3.0)
    sc = inp["scene"]
    W, H = inp["W"], inp["H"]
    leaf = lambda t: t.to(DEV).clone().contiguous().requires_grad_(True)
    tp, sh, lg = leaf(inp["tetpoints"]), leaf(inp["shs"]), leaf(torch.logit(inp["opacities"].clamp(1e-4, 1 - 1e-4)))
    consts = [sc["tetras"].to(DEV), sc["tetra_id"].to(DEV), sc["barys"].to(DEV), inp["canon_grad"].to(DEV), inp["scales"].to(DEV),
              sc["rotation"].to(DEV)]
    bg = torch.ones(3, device=DEV)
    cams = [syn.make_batch(W, H, azimuth=0.4), syn.make_batch(W, H, azimuth=0.4, fill=20.0)]
    targets = [torch.rand(3, H, W, generator=torch.Generator().manual_seed(60 + v)).to(DEV) for v in range(2)]
    params = (tp, sh, lg)

    def step(batch, target):
        means, cov6 = cage_deform(tp, *consts)
        img = render(batch, {"means3D": means, "cov3D_precomp": cov6, "opacity_logits": lg, "shs": sh, "rgb": None, "sh_degree": 3}, bg)["render"]
        loss = l1_loss(img, target)
        loss.backward()
        return img.detach(), loss.detach()

    eager, dmax, visible = [], 0, []
    for b, t in zip(cams, targets):
        for p in params:
            p.grad = None
        img, loss = step(b, t)
        start, plist, _ = R.last_tile_lists(W, H)
        eager.append((img.clone(), float(loss), [p.grad.clone() for p in params], _np(start), _np(plist)))
        dmax = max(dmax, R.last_counters()["D"])
        seen = np.zeros(inp["means3D"].shape[0], bool)
        seen[_np(plist)] = True
        visible.append(np.add.reduceat(seen, np.arange(0, seen.size, 64)) > 0)         # per wavefront: anything in a list
    assert int((visible[0] & ~visible[1]).sum()) >= 5, "camera B empties no wavefront of camera A"
    R.set_capacity_policy("static", int(1.25 * dmax) + 4096)
    try:
        slot = CameraSlot(W, H, device=DEV).set(cams[0])
        target = targets[0].clone()
        slot_batch = dict(cams[0], camera_slot=slot)
        for p in params:
            p.grad = None
        cap = CapturedStep(lambda: step(slot_batch, target), params=params, slots={"target": target}, camera=slot)
        for v in (1, 0, 1, 1, 0):
            img_g, loss_g = cap.replay(camera=cams[v], target=targets[v])
            torch.cuda.synchronize()
            cnt = R.last_counters()
            img_e, loss_e, grads_e, start_e, plist_e = eager[v]
            assert not cnt["overflow"] and cnt["D"] == int(start_e[-1])
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


def test_windowed_views_against_the_oracle():
    """Two windowed views of different crops in one batch (the window of each cuts the boxes of the wavefronts along its edges).
    The list of window tile (tx, ty) of view v is the oracle's list, on that view's padded raster, of tile (tx + ox / 16,
    ty + oy / 16) -- same Gaussians, same order, as records v P + i -- and empty outside the raster; D and the visible count follow."""
    from d3ga_amd import _lib
    from d3ga_amd import rasterizer as R
    from d3ga_amd.cameras import crop_window
    from d3ga_amd.renderer import render_views
    W, H, k = 161, 143, 2
    inps = [scene_inputs("T1", scale_mult=3.0, cx=57, cy=96, width=W, height=H), scene_inputs("T1", scale_mult=3.0, cx=120, cy=53, width=W, height=H, azimuth=1.3)]
    g = _take(inps[0], torch.arange(1000) * 3)
    P = g["P"]
    bg = torch.tensor([0.3, 0.6, 0.1])
    pkg = {"means3D": g["means3D"].to(DEV), "cov3D_precomp": g["cov6"].to(DEV), "opacities": g["opacities"].to(DEV), "shs": g["shs"].to(DEV),
           "rgb": None, "sh_degree": 3}
    with torch.no_grad():
        out = render_views([i["batch"] for i in inps], pkg, bg.to(DEV))["render"]
    assert tuple(out.shape) == (k, 3, H, W)
    binning, cap = R._last[torch.cuda.current_device()]
    off = (ctypes.c_int64 * 7)()
    assert _lib.lib().d3ga_raster_binning_layout_window(W, H, k, cap, off) == 0
    gx, gy = (W + 15) // 16 + 1, (H + 15) // 16 + 1
    tiles = gx * gy * k
    start = _np(binning[off[2]:off[2] + 4 * (tiles + 1)].view(torch.int32).long() & 0xFFFFFFFF)
    plist = _np(binning[off[5]:off[5] + 4 * int(start[-1])].view(torch.int32).long())
    want, want_start, visible = [], [0], 0
    for v, inp in enumerate(inps):
        w, h, ox, oy, W2, H2 = crop_window(inp["batch"])
        assert (W2, H2, w, h) == (W, H, inp["W"], inp["H"])
        ostart, olist, D_full, _ = _oracle(g, inp, bg)
        gxf, gyf = (w + 15) // 16, (h + 15) // 16
        seen = set()
        for ty in range(gy):
            for tx in range(gx):
                fx, fy = tx + ox // 16, ty + oy // 16
                lst = olist[ostart[fy * gxf + fx]:ostart[fy * gxf + fx + 1]] if fx < gxf and fy < gyf else olist[:0]
                want.append(lst + v * P)
                want_start.append(want_start[-1] + len(lst))
                seen.update(lst.tolist())
        assert 0 < want_start[-1] - want_start[-1 - gx * gy] < D_full, "the window cuts nothing away"
        visible += len(seen)
    np.testing.assert_array_equal(start, np.asarray(want_start))
    np.testing.assert_array_equal(plist, np.concatenate(want))
    cnt = R.last_counters()
    assert (cnt["D"], cnt["overflow"], cnt["visible"]) == (want_start[-1], False, visible), cnt
