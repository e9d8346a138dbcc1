"""Crop-window rasterization (include/d3ga.h: D3GA_CAMERA_SLOT_WINDOWED).  The reference renders every frame at a padded raster
size w x h that centres the principal point (lib/batch.py:186-198) and pastes the W x H window back out (renderer.py:36-47).
Claim under test: rendering the window directly IS `paste(render(batch))` -- images bit-identical (RGB, the pair's second image,
the inverse depth), radii bit-identical, the fused L1 loss equal to `l1_loss(paste(render), target)` up to its summation order,
gradients (means2D included) equal up to the summation order of the compositing backward's float atomics -- for one view, for
batches of views of different raster sizes and crops, and through a windowed camera slot that is re-pointed between cameras."""
import math
import os

import numpy as np
import pytest
import torch

from util import scene_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR = 2e-5          # max |a - b| / max |a| per leaf: the same-arithmetic bar of the view-batched tests (precomputed covariances)

# (W, H, cx, cy): every branch of paste() -- window at the left / right, top / bottom of the padded raster -- offsets of 0 to 47
# pixels, window sizes that are not multiples of 16, and a centred crop
CROPS = [(200, 152, 78, 60), (200, 152, 122, 95), (197, 150, 120, 53), (203, 149, 80, 101), (190, 170, 95, 85), (161, 143, 57, 96)]


def _leaf(t):
    return t.to(DEV).clone().contiguous().requires_grad_(True)


def _close(a, b, what, bar=BAR):
    scale = float(a.abs().max())
    err = float((a - b).abs().max())
    assert scale > 0 and err <= bar * scale, (what, err / max(scale, 1e-30))


def _inputs(W, H, cx, cy, azimuth=0.4):
    return scene_inputs("T1", scale_mult=3.0, cx=cx, cy=cy, width=W, height=H, azimuth=azimuth)


def _pkg(L, sh=True):
    return {"means3D": L["means3D"], "cov3D_precomp": L["cov6"], "opacities": L["opacities"], "shs": L["shs"] if sh else None,
            "rgb": None if sh else L["rgb"], "sh_degree": 3 if sh else 0}


def _leaves(inp, sh=True):
    return {k: _leaf(inp[k]) for k in (("means3D", "cov6", "opacities", "shs") if sh else ("means3D", "cov6", "opacities", "rgb"))}


def test_crop_window_mapping_covers_every_paste_branch():
    from d3ga_amd.cameras import crop_window
    seen = set()
    for W, H, cx, cy in CROPS:
        w, h, ox, oy, W2, H2 = crop_window(_inputs(W, H, cx, cy)["batch"])
        seen.add((ox == 0, oy == 0))
        assert (W2, H2) == (W, H) and 0 <= ox <= 47 and 0 <= oy <= 47
    assert seen == {(True, True), (True, False), (False, True), (False, False)}


@pytest.mark.parametrize("W,H,cx,cy", CROPS)
def test_single_view_window_equals_render_and_paste(W, H, cx, cy):
    from d3ga_amd.renderer import paste, render
    inp = _inputs(W, H, cx, cy)
    crop = inp["batch"]["crop"]
    bg = torch.tensor([0.3, 0.6, 0.1], device=DEV)
    gpix = torch.randn(3, H, W, generator=torch.Generator().manual_seed(3)).to(DEV)
    outs = []
    for cw in (False, True):
        L = _leaves(inp)
        pkg = _pkg(L)
        img = render(inp["batch"], pkg, bg, crop_window=cw)["render"]
        assert tuple(img.shape) == (3, H, W)
        (img * gpix).sum().backward()
        outs.append((img.detach(), L))
    torch.cuda.synchronize()
    (a, La), (b, Lb) = outs
    assert torch.equal(a, b), float((a - b).abs().max())
    assert float((a - bg.view(3, 1, 1)).abs().max()) > 0.05
    for k in La:
        _close(La[k].grad, Lb[k].grad, k)


@pytest.mark.parametrize("W,H,cx,cy", CROPS[:4])
def test_radii_means2d_and_inverse_depth_equal_the_full_raster(W, H, cx, cy):
    """The rasterizer operator itself: full raster (w x h) + paste against the windowed camera row -- radii bit for bit, the
    inverse-depth image bit for bit and its gradient, dL/dmeans2D within the bar."""
    from d3ga_amd import rasterizer as R
    from d3ga_amd.cameras import CAMERA_SLOT_WINDOWED, batch_to_camera, window_camera
    from d3ga_amd.renderer import paste
    inp = _inputs(W, H, cx, cy)
    batch = inp["batch"]
    crop = batch["crop"]
    bg = torch.tensor([0.9, 0.8, 0.7], device=DEV)
    cam = batch_to_camera(batch, device=DEV)
    mats, row = window_camera(batch, device=DEV)
    full = R.GaussianRasterizationSettings(int(batch["height"]), int(batch["width"]), cam.tanfovx, cam.tanfovy, bg, 1.0,
                                           cam.world_view_transform, cam.full_proj_transform, 3, cam.camera_center, False, False)
    win = R.GaussianRasterizationSettings(H, W, CAMERA_SLOT_WINDOWED, CAMERA_SLOT_WINDOWED, bg, 1.0, mats[0:16].view(4, 4),
                                          mats[32:48].view(4, 4), 3, row, False, False)
    g = torch.Generator().manual_seed(5)
    gpix, gd = torch.randn(3, H, W, generator=g).to(DEV), torch.randn(1, H, W, generator=g).to(DEV)
    res = []
    for s, cut in ((full, True), (win, False)):
        L = _leaves(inp)
        m2 = torch.zeros_like(L["means3D"], requires_grad=True)
        col, radii, invd = R.rasterize_gaussians(L["means3D"], m2, L["shs"], None, L["opacities"], None, None, L["cov6"], s)
        if cut:
            col, invd = paste(col, crop), paste(invd, crop)
        ((col * gpix).sum() + (invd * gd).sum()).backward()
        res.append((col.detach(), radii, invd.detach(), m2.grad, L))
    torch.cuda.synchronize()
    (ca, ra, ia, ma, La), (cb, rb, ib, mb, Lb) = res
    assert torch.equal(ca, cb) and torch.equal(ra, rb) and torch.equal(ia, ib)
    _close(ma, mb, "means2D")
    for k in La:
        _close(La[k].grad, Lb[k].grad, k)


@pytest.mark.parametrize("W,H,cx,cy", CROPS[:3])
def test_pair_and_fused_l1_through_the_window(W, H, cx, cy):
    from d3ga_amd.losses import l1_loss
    from d3ga_amd.renderer import render, render_l1, render_pair
    inp = _inputs(W, H, cx, cy)
    batch = inp["batch"]
    bg, bg0 = torch.tensor([0.2, 0.4, 0.9], device=DEV), torch.zeros(3, device=DEV)
    sil = torch.ones(inp["means3D"].shape[0], 3, device=DEV)
    g = torch.Generator().manual_seed(7)
    target = torch.rand(3, H, W, generator=g).to(DEV)
    gp, gp2 = torch.randn(3, H, W, generator=g).to(DEV), torch.randn(3, H, W, generator=g).to(DEV)
    # the pair
    A, B = _leaves(inp), _leaves(inp)
    pa = render_pair(batch, _pkg(A), bg, sil, bg0)
    pb = render_pair(batch, _pkg(B), bg, sil, bg0, crop_window=True)
    ((pa["render"] * gp).sum() + (pa["render2"] * gp2).sum()).backward()
    ((pb["render"] * gp).sum() + (pb["render2"] * gp2).sum()).backward()
    torch.cuda.synchronize()
    assert torch.equal(pa["render"], pb["render"]) and torch.equal(pa["render2"], pb["render2"])
    for k in A:
        _close(A[k].grad, B[k].grad, ("pair", k))
    # the fused L1: one operator on the window against render + paste + l1_loss
    A, B = _leaves(inp), _leaves(inp)
    img = render(batch, _pkg(A), bg)["render"]
    la = l1_loss(img, target)
    la.backward()
    out = render_l1(batch, _pkg(B), bg, target, crop_window=True)
    out["l1"].backward()
    torch.cuda.synchronize()
    assert torch.equal(out["render"], img)
    assert abs(float(out["l1"]) - float(la)) <= 1e-6 * abs(float(la))
    for k in A:
        _close(A[k].grad, B[k].grad, ("l1", k), 2e-4)       # (the bar of test_render_l1_equals_render_plus_l1_loss)


def _mixed_batches(k, W, H, seed):
    """k cameras around the body, each with its own principal point (so its own raster size and window offset), all pasting to W x H."""
    from d3ga_amd import synthetic as syn
    rng = np.random.default_rng(seed)
    out = []
    for v in range(k):
        cx, cy = int(rng.integers(W // 2 - 40, W // 2 + 41)), int(rng.integers(H // 2 - 40, H // 2 + 41))
        out.append(syn.make_batch(W, H, azimuth=0.4 + 2 * math.pi * v / max(k, 3), camera_id=v, cx=cx, cy=cy))
    return out


@pytest.mark.parametrize("k,sh", [(2, True), (5, False), (9, True)])
def test_k_cameras_of_mixed_raster_sizes(k, sh):
    from d3ga_amd.renderer import render, render_views
    inp = scene_inputs("T1", scale_mult=3.0)
    W, H = 197, 163
    batches = _mixed_batches(k, W, H, 11 + k)
    assert len({(b["width"], b["height"]) for b in batches}) > 1
    bg = torch.tensor([0.3, 0.6, 0.1], device=DEV)
    gpix = torch.randn(k, 3, H, W, generator=torch.Generator().manual_seed(k)).to(DEV)
    A = _leaves(inp, sh)
    imgs = []
    for v, b in enumerate(batches):
        img = render(b, _pkg(A, sh), bg)["render"]
        (img * gpix[v]).sum().backward()
        imgs.append(img.detach())
    B = _leaves(inp, sh)
    out = render_views(batches, _pkg(B, sh), bg)["render"]
    (out * gpix).sum().backward()
    torch.cuda.synchronize()
    assert tuple(out.shape) == (k, 3, H, W)
    for v in range(k):
        assert torch.equal(out[v], imgs[v]), (v, float((out[v] - imgs[v]).abs().max()))
    for n in A:
        _close(A[n].grad, B[n].grad, n)


@pytest.mark.parametrize("mode", ["images", "l1", "pair"])
def test_colorfield_batch_of_frames_with_crops(mode):
    """The ColorField configuration's batch of frames (own pose, colours, opacities and background per frame) from cameras with
    different crops, against render / render_l1 / render_pair + paste per frame."""
    from d3ga_amd.losses import l1_loss
    from d3ga_amd.renderer import render, render_pair, render_views
    inp = scene_inputs("T1", scale_mult=3.0)
    k, W, H = 4, 190, 171
    batches = _mixed_batches(k, W, H, 29)
    g = torch.Generator().manual_seed(41)
    P = inp["means3D"].shape[0]
    bg = torch.rand(k, 3, generator=g).to(DEV)
    bg0 = torch.zeros(3, device=DEV)
    sil = torch.ones(P, 3, device=DEV)
    means0 = inp["means3D"].unsqueeze(0) + 0.02 * torch.randn(k, P, 3, generator=g)
    cov0 = torch.stack([inp["cov6"] * (1.0 + 0.05 * v) for v in range(k)])
    rgb0 = (inp["rgb"].unsqueeze(0) * (0.6 + 0.8 * torch.rand(k, P, 3, generator=g))).clamp(0.0, 1.0)
    op0 = (inp["opacities"].reshape(1, P, 1) * (0.5 + torch.rand(k, P, 1, generator=g))).clamp(0.02, 0.98)
    gp, gp2 = torch.randn(k, 3, H, W, generator=g).to(DEV), torch.randn(k, 3, H, W, generator=g).to(DEV)
    targets = torch.rand(k, 3, H, W, generator=g).to(DEV)

    def leaves():
        return [_leaf(t) for t in (means0, cov0, rgb0, op0)]

    def frames(L):
        return [{"means3D": L[0][v], "cov3D_precomp": L[1][v], "rgb": L[2][v], "opacities": L[3][v], "shs": None, "sh_degree": 0}
                for v in range(k)]

    A = leaves()
    imgs, imgs2, loss_a = [], [], 0.0
    for v, pk in enumerate(frames(A)):
        if mode == "pair":
            o = render_pair(batches[v], pk, bg[v], sil, bg0)
            ((o["render"] * gp[v]).sum() + (o["render2"] * gp2[v]).sum()).backward()
            imgs2.append(o["render2"].detach())
            img = o["render"]
        else:
            img = render(batches[v], pk, bg[v])["render"]
            if mode == "l1":
                lv = l1_loss(img, targets[v]) / k
                lv.backward()
                loss_a += float(lv)
            else:
                (img * gp[v]).sum().backward()
        imgs.append(img.detach())
    B = leaves()
    if mode == "pair":
        o = render_views(batches, frames(B), bg, colors2=sil, bg_color2=bg0)
        ((o["render"] * gp).sum() + (o["render2"] * gp2).sum()).backward()
    elif mode == "l1":
        o = render_views(batches, frames(B), bg, targets=targets)
        o["l1"].backward()
        assert abs(float(o["l1"]) - loss_a) <= 1e-5 * abs(loss_a)
    else:
        o = render_views(batches, frames(B), bg)
        (o["render"] * gp).sum().backward()
    torch.cuda.synchronize()
    for v in range(k):
        assert torch.equal(o["render"][v], imgs[v]), (v, float((o["render"][v] - imgs[v]).abs().max()))
        if mode == "pair":
            assert torch.equal(o["render2"][v], imgs2[v])
    for n in range(4):
        _close(A[n].grad, B[n].grad, (mode, n), BAR if mode != "l1" else 2e-4)


def test_windowed_camera_slot_follows_cameras_of_any_raster_size():
    """One windowed CameraSlot (CameraSlot.windowed(W, H)), re-pointed with set() at 8 cameras of different raster sizes that all
    paste to W x H: every render equals render + paste of that camera, bit for bit, gradients within the bar."""
    from d3ga_amd.cameras import CameraSlot
    from d3ga_amd.renderer import render, render_l1
    inp = scene_inputs("T1", scale_mult=3.0)
    W, H = 185, 158
    batches = _mixed_batches(8, W, H, 3)
    slot = CameraSlot.windowed(W, H, device=DEV)
    bg = torch.tensor([0.5, 0.5, 0.5], device=DEV)
    target = torch.rand(3, H, W, generator=torch.Generator().manual_seed(2)).to(DEV)
    for b in batches:
        A, B = _leaves(inp), _leaves(inp)
        ref = render_l1(b, _pkg(A), bg, target, crop_window=True)
        slot.set(b)
        mine = render_l1(dict(b, camera_slot=slot), _pkg(B), bg, target)
        ref["l1"].backward()
        mine["l1"].backward()
        torch.cuda.synchronize()
        assert torch.equal(ref["render"], mine["render"]) and float(ref["l1"]) == float(mine["l1"])
        full = render(b, _pkg(_leaves(inp)), bg)["render"].detach()
        assert torch.equal(full, mine["render"])
        for n in A:
            _close(A[n].grad, B[n].grad, n)


def test_captured_step_replays_over_cameras_of_mixed_raster_sizes():
    """A training step (windowed slot + fused L1) captured ONCE in a hipGraph and replayed with 8 cameras of different raster sizes:
    images bit-identical to the eager render + paste, gradients within the bar."""
    from d3ga_amd import rasterizer as R
    from d3ga_amd.cameras import CameraSlot
    from d3ga_amd.renderer import render, render_l1
    inp = scene_inputs("T1", scale_mult=3.0)
    W, H = 185, 158
    batches = _mixed_batches(8, W, H, 5)
    bg = torch.tensor([0.5, 0.5, 0.5], device=DEV)
    target = torch.rand(3, H, W, generator=torch.Generator().manual_seed(2)).to(DEV)
    slot = CameraSlot.windowed(W, H, device=DEV)
    B = _leaves(inp)
    out_img = torch.empty(3, H, W, device=DEV)
    R.set_capacity_policy("static", 1 << 20)
    try:
        def step():
            for t in B.values():
                t.grad = None
            o = render_l1(dict(batches[0], camera_slot=slot), _pkg(B), bg, target)
            o["l1"].backward()
            out_img.copy_(o["render"].detach())
        slot.set(batches[0])
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            step()                                          # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        for t in B.values():
            t.grad = None
        with torch.cuda.graph(graph):
            step()
        grads = {n: t.grad for n, t in B.items()}
        for b in batches:
            slot.set(b)
            graph.replay()
            torch.cuda.synchronize()
            assert not R.last_counters()["overflow"]
            A = _leaves(inp)
            img = render(b, _pkg(A), bg)["render"]
            from d3ga_amd.losses import l1_loss
            l1_loss(img, target).backward()
            torch.cuda.synchronize()
            assert torch.equal(img, out_img)
            for n in A:
                _close(A[n].grad, grads[n], n, 2e-4)
    finally:
        R.set_capacity_policy("auto")


def test_nan_view_is_contained_in_a_windowed_batch():
    from d3ga_amd.renderer import render, render_views
    inp = scene_inputs("T1", scale_mult=3.0)
    k, W, H = 3, 176, 150
    batches = _mixed_batches(k, W, H, 8)
    P = inp["means3D"].shape[0]
    means = inp["means3D"].unsqueeze(0).repeat(k, 1, 1)
    means[1, :7] = float("nan")
    means[1, 7:11] = float("inf")
    bg = torch.tensor([0.3, 0.3, 0.3], device=DEV)
    imgs = []
    with torch.no_grad():
        for v in range(k):
            imgs.append(render(batches[v], {"means3D": means[v].to(DEV), "cov3D_precomp": inp["cov6"].to(DEV),
                                            "opacities": inp["opacities"].to(DEV), "shs": None, "rgb": inp["rgb"].to(DEV),
                                            "sh_degree": 0}, bg)["render"])
        frames = [{"means3D": means[v].to(DEV), "cov3D_precomp": inp["cov6"].to(DEV), "opacities": inp["opacities"].to(DEV),
                   "shs": None, "rgb": inp["rgb"].to(DEV), "sh_degree": 0} for v in range(k)]
        out = render_views(batches, frames, bg)["render"]
    for v in range(k):
        assert torch.equal(out[v], imgs[v]) and bool(torch.isfinite(out[v]).all())


def test_actor02_shaped_window():
    """actor02-shaped: 135k Gaussians, a 747 x 1022 pasted window of an off-centre camera."""
    from d3ga_amd.renderer import render, render_l1
    from d3ga_amd import synthetic as syn
    inp = scene_inputs("C3")
    P = inp["means3D"].shape[0]
    n = min(P, 135_000)
    b = syn.make_batch(747, 1022, cx=351, cy=540, fill=0.85)
    bg = torch.tensor([1.0, 1.0, 1.0], device=DEV)
    target = torch.rand(3, 1022, 747, generator=torch.Generator().manual_seed(1)).to(DEV)
    L = {k: inp[k][:n] for k in ("means3D", "cov6", "opacities", "shs")}
    A, B = ({k: _leaf(t) for k, t in L.items()} for _ in range(2))
    img = render(b, _pkg(A), bg)["render"]
    from d3ga_amd.losses import l1_loss
    l1_loss(img, target).backward()
    out = render_l1(b, _pkg(B), bg, target, crop_window=True)
    out["l1"].backward()
    torch.cuda.synchronize()
    assert torch.equal(out["render"], img)
    for k in A:
        _close(A[k].grad, B[k].grad, k, 2e-4)


@pytest.mark.parametrize("seed", range(int(os.environ.get("D3GA_CROP_FUZZ_N", "12"))))
def test_crop_window_fuzz(seed):
    """Random k (1..6), window sizes, principal points, SH or precomputed colours, frames or cameras: windowed render_views /
    render(crop_window=True) against render + paste per view.  D3GA_CROP_FUZZ_N sets the campaign size."""
    from d3ga_amd.renderer import render, render_views
    rng = np.random.default_rng(1000 + seed)
    k = int(rng.integers(1, 7))
    W, H = int(rng.integers(64, 260)), int(rng.integers(64, 260))
    sh = bool(rng.integers(2))
    per_frame = bool(rng.integers(2)) and k > 1
    inp = scene_inputs("T1", scale_mult=float(rng.uniform(1.0, 4.0)), seed=17 + seed % 3)
    batches = _mixed_batches(k, W, H, seed)
    bg = torch.tensor(rng.uniform(0, 1, 3).astype(np.float32), device=DEV)
    gp = torch.randn(k, 3, H, W, generator=torch.Generator().manual_seed(seed)).to(DEV)
    shift = torch.from_numpy(rng.normal(0, 0.01, (k,) + tuple(inp["means3D"].shape)).astype(np.float32))
    A, B = _leaves(inp, sh), _leaves(inp, sh)

    def frames(L):
        return [dict(_pkg(L, sh), means3D=L["means3D"] + shift[v].to(DEV)) for v in range(k)]
    imgs = []
    for v, b in enumerate(batches):
        pk = frames(A)[v] if per_frame else _pkg(A, sh)
        img = render(b, pk, bg)["render"]
        (img * gp[v]).sum().backward()
        imgs.append(img.detach())
    if k == 1:
        out = render(batches[0], _pkg(B, sh), bg, crop_window=True)["render"].unsqueeze(0)
    else:
        out = render_views(batches, frames(B) if per_frame else _pkg(B, sh), bg)["render"]
    (out * gp).sum().backward()
    torch.cuda.synchronize()
    for v in range(k):
        assert torch.equal(out[v], imgs[v]), (seed, v)
    for n in A:
        _close(A[n].grad, B[n].grad, (seed, n), 2e-4)
