"""Per-view appearance and backgrounds for view-batched rendering (include/d3ga.h: d3ga_raster_params::per_view_appearance,
::per_view_background): the reference's main configurations (use_shs: false) compute every Gaussian's colour and opacity per frame
with ColorField (models/cage_net.py:232-258) and draw a new background per frame (models/trainer.py:95-100).  Claim under test:
every view of a batch with its own colours, opacities and background IS the single-view render of that view with those inputs --
images bit-identical, the per-view colour and opacity gradients those of the single-view backward, the gradients of shared inputs
their sum over the views."""
import copy
import ctypes
import math

import pytest
import torch

from util import scene_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _order_bar(from_sr):
    """Bar of the same-arithmetic comparisons (max |a - b| / max |a| per leaf), as in the other view-batched tests: both sides form
    the same sums, the float atomics of the compositing backward landing in another order.  With (scales, rotations) the
    operator's own run-to-run spread reaches 6.4e-5 (tools/diag_spread.py)."""
    return 2e-4 if from_sr else 2e-5


def _batches(inp, k, fov_jitter=False):
    from d3ga_amd import synthetic as syn
    out = []
    for v in range(k):
        b = syn.make_batch(inp["W"], inp["H"], azimuth=0.4 + 2 * math.pi * v / max(k, 3), camera_id=v,
                           fill=0.85 * (1.0 + (0.1 * v if fov_jitter else 0.0)))
        out.append(b)
    return out


def _settings(inp, batch, bg, sh_degree=0):
    from d3ga_amd import rasterizer as R
    from d3ga_amd.cameras import batch_to_camera
    cam = batch_to_camera(batch, device=DEV)
    return R.GaussianRasterizationSettings(
        image_height=inp["H"], image_width=inp["W"], tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=bg, scale_modifier=1.0,
        viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, sh_degree=sh_degree, campos=cam.camera_center,
        prefiltered=False, debug=False, antialiasing=False)


def _appearance(inp, k, seed, logits):
    """Per-view colours (k,P,3) and opacities (k,P,1): view v's are the scene's, moved per view (what ColorField does with the
    view direction and the frame encoding)."""
    g = torch.Generator().manual_seed(seed)
    P = inp["means3D"].shape[0]
    rgb = (inp["rgb"].unsqueeze(0) * (0.6 + 0.8 * torch.rand(k, P, 3, generator=g))).clamp(0.0, 1.0)
    op = (inp["opacities"].reshape(1, P, 1) * (0.5 + torch.rand(k, P, 1, generator=g))).clamp(0.02, 0.98)
    return rgb, (torch.log(op) - torch.log1p(-op)) if logits else op


def _leaf(t):
    return t.to(DEV).clone().contiguous().requires_grad_(True)


def _geometry(inp, from_sr):
    d = {"means3D": inp["means3D"]}
    d.update({"scales": inp["scales"], "rots": inp["scene"]["rotation"]} if from_sr else {"cov6": inp["cov6"]})
    return {n: _leaf(t) for n, t in d.items()}


def _close(a, b, bar, what):
    scale = float(a.abs().max())
    err = float((a - b).abs().max())
    assert scale > 0 and err <= bar * scale, (what, err / max(scale, 1e-30))


@pytest.mark.parametrize("k,from_sr,logits", [(2, False, False), (5, True, True), (9, False, True), (9, True, False)])
def test_k_cameras_with_per_view_colours_and_opacities(k, from_sr, logits):
    """k cameras of one pose, rgb (k,P,3) and opacities (k,P,1) -- activated or logits -- against k single-view renders with that
    view's colours and opacities.  k = 9: the second kMaxGroup group of the per-Gaussian backward writes only its own views."""
    from d3ga_amd import rasterizer as R
    from d3ga_amd.raster_views import CameraBatch, rasterize_gaussians_views
    inp = scene_inputs("T1", scale_mult=3.0)
    batches = _batches(inp, k, fov_jitter=True)
    bg = torch.tensor([0.3, 0.6, 0.1], device=DEV)
    rgb0, op0 = _appearance(inp, k, 5 + k, logits)
    act = "sigmoid" if logits else None
    g = torch.Generator().manual_seed(3)
    gpix = torch.randn(k, 3, inp["H"], inp["W"], generator=g).to(DEV)

    ref, rgb_r, op_r = _geometry(inp, from_sr), _leaf(rgb0), _leaf(op0)
    imgs = []
    for v, b in enumerate(batches):
        img = R.rasterize_gaussians(ref["means3D"], None, None, rgb_r[v], op_r[v], ref.get("scales"), ref.get("rots"), ref.get("cov6"),
                                    _settings(inp, b, bg), None, act, want_invdepth=False)[0]
        (img * gpix[v]).sum().backward()
        imgs.append(img.detach())
    mine, rgb_m, op_m = _geometry(inp, from_sr), _leaf(rgb0), _leaf(op0)
    cams = CameraBatch(k, inp["W"], inp["H"], device=DEV).set(batches)
    colors, radii = rasterize_gaussians_views(mine["means3D"], None, rgb_m, op_m, mine.get("scales"), mine.get("rots"), mine.get("cov6"),
                                              cams, bg, opacity_activation=act)
    (colors * gpix).sum().backward()
    torch.cuda.synchronize()
    for v in range(k):
        assert torch.equal(colors[v], imgs[v]), (v, float((colors[v] - imgs[v]).abs().max()))
        assert float((colors[v] - bg.view(3, 1, 1)).abs().max()) > 0.05
        _close(rgb_r.grad[v], rgb_m.grad[v], 2e-5, ("rgb", v))
        _close(op_r.grad[v], op_m.grad[v], 2e-5, ("opacity", v))
    assert rgb_m.grad.shape == (k, inp["means3D"].shape[0], 3) and op_m.grad.shape == op0.shape
    for n in ref:
        _close(ref[n].grad, mine[n].grad, _order_bar(from_sr), n)


def _frame_packages(geo, rgb, op, k):
    return [{"means3D": geo["means3D"][v], "cov3D_precomp": geo["cov6"][v], "opacities": op[v], "rgb": rgb[v], "shs": None,
             "sh_degree": 0} for v in range(k)]


@pytest.mark.parametrize("mode", ["images", "l1", "pair"])
def test_batch_of_frames_with_per_frame_appearance_and_backgrounds(mode):
    """per_view_geometry + per_view_appearance + per_view_background through renderer.render_views with a LIST of packages (own
    pose, colours and opacities per frame) and a random background per frame, against render / render_l1 / render_pair per frame:
    images alone, the fused L1 loss, and the RGB + silhouette pair (colors2 shared, bg_color2 black)."""
    from d3ga_amd.renderer import render, render_l1, render_pair, render_views
    inp = scene_inputs("T1", scale_mult=3.0)
    k = 4
    batches = _batches(inp, k)
    g = torch.Generator().manual_seed(41)
    P = inp["means3D"].shape[0]
    bg = torch.rand(k, 3, generator=g).to(DEV)                       # models/trainer.py:95-100: np.random.rand(3) per frame
    bg0 = torch.zeros(3, device=DEV)
    sil = torch.ones(P, 3, device=DEV)
    shift = 0.02 * torch.randn(k, P, 3, generator=g)
    geo0 = {"means3D": inp["means3D"].unsqueeze(0) + shift, "cov6": torch.stack([inp["cov6"] * (1.0 + 0.05 * v) for v in range(k)])}
    rgb0, op0 = _appearance(inp, k, 43, False)
    gp, gp2 = torch.randn(k, 3, inp["H"], inp["W"], generator=g).to(DEV), torch.randn(k, 3, inp["H"], inp["W"], generator=g).to(DEV)
    targets = torch.rand(k, 3, inp["H"], inp["W"], generator=g).to(DEV)

    def leaves():
        return {n: _leaf(t) for n, t in geo0.items()}, _leaf(rgb0), _leaf(op0)

    ref, rgb_r, op_r = leaves()
    imgs, imgs2, losses = [], [], []
    for v, pk in enumerate(_frame_packages(ref, rgb_r, op_r, k)):
        if mode == "images":
            img = render(batches[v], pk, bg[v])["render"]
            (img * gp[v]).sum().backward()
        elif mode == "l1":
            out = render_l1(batches[v], pk, bg[v], targets[v])
            img = out["render"]
            losses.append(out["l1"])
        else:
            both = render_pair(batches[v], pk, bg[v], sil, bg0)
            img = both["render"]
            ((img * gp[v]).sum() + (both["render2"] * gp2[v]).sum()).backward()
            imgs2.append(both["render2"].detach())
        imgs.append(img.detach())
    if mode == "l1":
        loss_ref = torch.stack(losses).mean()                         # train.py:218-221: the batch's losses averaged
        loss_ref.backward()

    mine, rgb_m, op_m = leaves()
    pkgs = _frame_packages(mine, rgb_m, op_m, k)
    if mode == "images":
        out = render_views(batches, pkgs, bg)
        (out["render"] * gp).sum().backward()
    elif mode == "l1":
        out = render_views(batches, pkgs, bg, targets=targets)
        out["l1"].backward()
    else:
        out = render_views(batches, pkgs, bg, colors2=sil, bg_color2=bg0)
        ((out["render"] * gp).sum() + (out["render2"] * gp2).sum()).backward()
    torch.cuda.synchronize()
    if mode == "l1":
        a, b = float(loss_ref), float(out["l1"])
        assert abs(a - b) <= 1e-6 * abs(a), (a, b)
    for v in range(k):
        assert torch.equal(out["render"][v], imgs[v]), v
        if mode == "pair":
            assert torch.equal(out["render2"][v], imgs2[v]), v
        _close(rgb_r.grad[v], rgb_m.grad[v], 2e-5, ("rgb", v))
        _close(op_r.grad[v], op_m.grad[v], 2e-5, ("opacity", v))
        for n in ref:
            _close(ref[n].grad[v], mine[n].grad[v], _order_bar(False), (n, v))


def test_per_view_backgrounds_with_shared_sh_appearance():
    """per_view_background alone: k cameras of one SH-coloured pose, bg (k,3); every image equals the single-view render with its
    own background, the gradients the sum over the views."""
    from d3ga_amd import rasterizer as R
    from d3ga_amd.raster_views import CameraBatch, rasterize_gaussians_views
    inp = scene_inputs("C1")
    k = 3
    batches = _batches(inp, k, fov_jitter=True)
    g = torch.Generator().manual_seed(61)
    bg = torch.rand(k, 3, generator=g).to(DEV)
    gpix = torch.randn(k, 3, inp["H"], inp["W"], generator=g).to(DEV)
    names = ("means3D", "cov6", "opacities", "shs")
    ref = {n: _leaf(inp[n]) for n in names}
    imgs = []
    for v, b in enumerate(batches):
        img = R.rasterize_gaussians(ref["means3D"], None, ref["shs"], None, ref["opacities"], None, None, ref["cov6"],
                                    _settings(inp, b, bg[v], 3), want_invdepth=False)[0]
        (img * gpix[v]).sum().backward()
        imgs.append(img.detach())
    mine = {n: _leaf(inp[n]) for n in names}
    cams = CameraBatch(k, inp["W"], inp["H"], device=DEV).set(batches)
    colors, _ = rasterize_gaussians_views(mine["means3D"], mine["shs"], None, mine["opacities"], None, None, mine["cov6"], cams, bg,
                                          sh_degree=3)
    (colors * gpix).sum().backward()
    torch.cuda.synchronize()
    for v in range(k):
        assert torch.equal(colors[v], imgs[v]), (v, float((colors[v] - imgs[v]).abs().max()))
    assert not torch.equal(colors[0][:, 0, 0], colors[1][:, 0, 0])          # the corners show the views' own backgrounds
    for n in names:
        _close(ref[n].grad, mine[n].grad, 2e-5, n)


def test_color_field_batch_of_frames_end_to_end():
    """The reference's ColorField training step over a batch of k = 4 frames (own pose, frame encoding, camera, background):
    ColorField per frame, ONE render_views with per-frame colours / opacities / backgrounds and the fused L1 -- against the
    sequential loop (render per frame, l1_loss, the mean over the batch, train.py:218-221)."""
    from d3ga_amd.cameras import batch_to_camera
    from d3ga_amd.losses import l1_loss
    from d3ga_amd.mlp import ColorField, view_directions
    from d3ga_amd.renderer import render, render_views
    inp = scene_inputs("T1", scale_mult=3.0)
    k = 4
    batches = _batches(inp, k)
    P = inp["means3D"].shape[0]
    torch.manual_seed(71)
    cf_ref = ColorField().to(DEV)
    cf_mine = copy.deepcopy(cf_ref)
    g = torch.Generator().manual_seed(73)
    feat0 = 0.33 * torch.rand(P, 64, generator=g)
    poses = [(0.3 * torch.randn(98, generator=g)).to(DEV) for _ in range(k)]
    enc0 = 0.1 * torch.randn(k, 32, generator=g)
    means = [(inp["means3D"] + 0.02 * torch.randn(P, 3, generator=g)).to(DEV) for _ in range(k)]
    cov6 = inp["cov6"].to(DEV)
    centres = [batch_to_camera(b, device=DEV).camera_center.reshape(1, 3) for b in batches]
    bg = torch.rand(k, 3, generator=g).to(DEV)
    targets = torch.rand(k, 3, inp["H"], inp["W"], generator=g).to(DEV)

    def packages(cf, feat, enc):
        out = []
        for v in range(k):
            rgb, opac = cf(feat, poses[v], view_directions(means[v], centres[v]), frame_encoding=enc[v])      # cage_net.py:232-258
            out.append({"means3D": means[v], "cov3D_precomp": cov6, "opacities": opac, "rgb": rgb, "shs": None, "sh_degree": 0})
        return out

    feat_r, enc_r = _leaf(feat0), _leaf(enc0)
    loss_r = torch.stack([l1_loss(render(batches[v], pk, bg[v])["render"], targets[v])
                          for v, pk in enumerate(packages(cf_ref, feat_r, enc_r))]).mean()
    loss_r.backward()
    feat_m, enc_m = _leaf(feat0), _leaf(enc0)
    loss_m = render_views(batches, packages(cf_mine, feat_m, enc_m), bg, targets=targets)["l1"]
    loss_m.backward()
    torch.cuda.synchronize()
    a, b = float(loss_r), float(loss_m)
    assert abs(a - b) <= 1e-6 * abs(a), (a, b)
    for (n, p), q in zip(cf_ref.named_parameters(), cf_mine.parameters()):
        _close(p.grad, q.grad, 1e-4, n)
    _close(feat_r.grad, feat_m.grad, 1e-4, "color_feat")
    for v in range(k):
        _close(enc_r.grad[v], enc_m.grad[v], 1e-4, ("frame_encoding", v))


def test_nan_and_inf_in_one_views_appearance_stay_in_that_view():
    """A NaN opacity in view 1 culls the Gaussian in view 1 only; an Inf colour in view 2 poisons view 2 only.  Batch of frames
    (nothing shared between the views): the other views' images are bit-identical to their single-view renders and every gradient
    they produce is finite and equals the single-view one."""
    from d3ga_amd.raster_views import CameraBatch, rasterize_gaussians_views
    from d3ga_amd.renderer import render
    inp = scene_inputs("T1", scale_mult=3.0)
    k = 4
    batches = _batches(inp, k, fov_jitter=True)
    P = inp["means3D"].shape[0]
    g = torch.Generator().manual_seed(81)
    bg = torch.rand(k, 3, generator=g).to(DEV)
    gpix = torch.randn(k, 3, inp["H"], inp["W"], generator=g).to(DEV)
    geo0 = {"means3D": inp["means3D"].unsqueeze(0) + 0.01 * torch.randn(k, P, 3, generator=g),
            "cov6": inp["cov6"].unsqueeze(0).expand(k, P, 6).contiguous()}
    rgb0, op0 = _appearance(inp, k, 83, False)
    cams = CameraBatch(k, inp["W"], inp["H"], device=DEV).set(batches)
    with torch.no_grad():                                              # two Gaussians every view sees
        _, radii = rasterize_gaussians_views(geo0["means3D"].to(DEV), None, rgb0.to(DEV), op0.to(DEV), None, None, geo0["cov6"].to(DEV),
                                             cams, bg)
    seen = torch.nonzero((radii > 0).all(0)).flatten().tolist()
    a, b = seen[len(seen) // 3], seen[2 * len(seen) // 3]
    op0[1, a] = float("nan")
    rgb0[2, b] = float("inf")

    def leaves():
        return {n: _leaf(t) for n, t in geo0.items()}, _leaf(rgb0), _leaf(op0)
    ref, rgb_r, op_r = leaves()
    imgs = []
    for v, pk in enumerate(_frame_packages(ref, rgb_r, op_r, k)):
        img = render(batches[v], pk, bg[v])["render"]
        (img * gpix[v]).sum().backward()
        imgs.append(img.detach())
    mine, rgb_m, op_m = leaves()
    colors, radii = rasterize_gaussians_views(mine["means3D"], None, rgb_m, op_m, None, None, mine["cov6"], cams, bg)
    (colors * gpix).sum().backward()
    torch.cuda.synchronize()
    assert int(radii[1, a]) == 0 and all(int(radii[v, a]) > 0 for v in (0, 2, 3))
    assert not bool(torch.isfinite(imgs[2]).all())                     # (the poison did reach view 2 of the reference)
    torch.testing.assert_close(colors[2], imgs[2], rtol=0, atol=0, equal_nan=True)
    for v in (0, 1, 3):
        assert bool(torch.isfinite(colors[v]).all()) and torch.equal(colors[v], imgs[v]), v
        for name, r, m in [("rgb", rgb_r.grad[v], rgb_m.grad[v]), ("opacity", op_r.grad[v], op_m.grad[v])] + \
                          [(n, ref[n].grad[v], mine[n].grad[v]) for n in ref]:
            assert bool(torch.isfinite(m).all()), (name, v)
            _close(r, m, 2e-5, (name, v))
    assert float(op_m.grad[1, a]) == 0.0 and float(rgb_m.grad[1, a].abs().max()) == 0.0      # culled in view 1: zero gradients there


def test_captured_color_field_step_replays_with_new_cameras_and_backgrounds():
    """The batched ColorField-configuration step (ColorField per camera, rgb (k,P,3) + opacities (k,P,1) in ONE package, a (k,3)
    background, fused L1, the whole backward) as one hipGraph, replayed with the cameras of its CameraBatch rewritten (CameraBatch.set)
    and new random backgrounds written in place into the same (k,3) tensor: every replay equals the eager step."""
    from d3ga_amd import rasterizer as R
    from d3ga_amd import synthetic as syn
    from d3ga_amd.graph import CapturedStep
    from d3ga_amd.mlp import ColorField, view_directions
    from d3ga_amd.raster_views import CameraBatch
    from d3ga_amd.renderer import render_views
    inp = scene_inputs("T1", scale_mult=3.0)
    k, W, H = 3, inp["W"], inp["H"]
    P = inp["means3D"].shape[0]
    cams_of = lambda r: [syn.make_batch(W, H, azimuth=0.3 + 0.7 * r + 2 * math.pi * v / 8, camera_id=v, fill=0.8 + 0.05 * v) for v in range(k)]
    cams = CameraBatch(k, W, H, device=DEV).set(cams_of(0))
    torch.manual_seed(91)
    cf = ColorField().to(DEV)
    feat = (0.33 * torch.rand(P, 64, device=DEV)).requires_grad_(True)
    enc = (0.1 * torch.randn(k, 32, device=DEV)).requires_grad_(True)
    pose = 0.3 * torch.randn(98, device=DEV)
    means, cov6 = _leaf(inp["means3D"]), _leaf(inp["cov6"])
    bg = torch.rand(k, 3, generator=torch.Generator().manual_seed(0)).to(DEV)
    targets = torch.rand(k, 3, H, W, generator=torch.Generator().manual_seed(0)).to(DEV)
    params = list(cf.parameters()) + [feat, enc, means, cov6]
    one = torch.ones((), device=DEV)

    def step():
        rgbs, ops = [], []
        for v in range(k):
            rgb, op = cf(feat, pose, view_directions(means, cams.campos[v, :3]), frame_encoding=enc[v])
            rgbs.append(rgb)
            ops.append(op)
        pkg = {"means3D": means, "cov3D_precomp": cov6, "rgb": torch.stack(rgbs), "opacities": torch.stack(ops), "shs": None, "sh_degree": 0}
        loss = render_views(None, pkg, bg, targets=targets, cameras=cams)["l1"]
        loss.backward(one)
        return loss

    def zero():
        for p in params:
            p.grad = None
    try:
        zero(); step()
        R.set_capacity_policy("static", int(R.last_counters()["D"] * 2.0) + 4096)
        zero()
        graph = CapturedStep(step, params=params, check_every=1)
        for r in range(1, 4):
            cams.set(cams_of(r))
            bg.copy_(torch.rand(k, 3, generator=torch.Generator().manual_seed(r)).to(DEV))
            targets.copy_(torch.rand(k, 3, H, W, generator=torch.Generator().manual_seed(r)).to(DEV))
            loss_g = graph.replay()
            torch.cuda.synchronize()
            static = [p.grad for p in params]
            got, lg = [x.clone() for x in static], float(loss_g.detach())
            zero()
            le = float(step())
            torch.cuda.synchronize()
            assert abs(lg - le) <= 1e-6 * abs(le), (r, lg, le)
            for p, x in zip(params, got):
                _close(p.grad, x, 1e-5, (r, tuple(p.shape)))
            for p, x in zip(params, static):
                p.grad = x
        assert graph.check_overflow()["D"] > 0
    finally:
        R.set_capacity_policy("auto")


def test_refusals_launch_nothing():
    """Each refusal is a ValueError raised before any launch: SH colours with per-view opacities, a leading dimension that is not
    k, the camera-sharded exchange (grad_sync) with per-view appearance, packages with different SH degrees.  The C entry points
    refuse SH colours with per_view_appearance (D3GA_E_CONFIG)."""
    from d3ga_amd import _lib, dist
    from d3ga_amd import rasterizer as R
    from d3ga_amd.raster_views import CameraBatch, rasterize_gaussians_views
    from d3ga_amd.renderer import render_views
    inp = scene_inputs("T1", scale_mult=3.0)
    k = 3
    batches = _batches(inp, k)
    P = inp["means3D"].shape[0]
    cams = CameraBatch(k, inp["W"], inp["H"], device=DEV).set(batches)
    means, cov6, shs = (inp[n].to(DEV) for n in ("means3D", "cov6", "shs"))
    rgb, op = (t.to(DEV) for t in _appearance(inp, k, 97, False))
    bg = torch.ones(3, device=DEV)
    torch.cuda.synchronize()
    last = R._last.get(torch.cuda.current_device())                   # (every batched forward leaves its binning buffer here)
    cases = [
        lambda: rasterize_gaussians_views(means, shs, None, op, None, None, cov6, cams, bg, sh_degree=3),
        lambda: rasterize_gaussians_views(means, None, torch.cat([rgb, rgb[:1]]), op, None, None, cov6, cams, bg),
        lambda: rasterize_gaussians_views(means, None, rgb, torch.cat([op, op[:1]]), None, None, cov6, cams, bg),
        lambda: rasterize_gaussians_views(means, None, rgb, op, None, None, cov6, cams, torch.ones(k + 1, 3, device=DEV)),
        lambda: rasterize_gaussians_views(means, None, rgb.requires_grad_(True), op, None, None, cov6, cams, bg,
                                          grad_sync=dist.ViewShardedGrads()),
        lambda: render_views(batches, [{"means3D": means, "cov3D_precomp": cov6, "opacities": op[v], "shs": shs, "rgb": None,
                                        "sh_degree": 3 - (v == 2)} for v in range(k)], bg),
    ]
    for i, case in enumerate(cases):
        with pytest.raises(ValueError) as e:
            case()
        if i == 4:
            assert "BucketedGradReducer" in str(e.value)
    torch.cuda.synchronize()
    cur = R._last.get(torch.cuda.current_device())
    assert cur is last, "a refused call ran the rasterizer"

    L = _lib.lib()
    buf = torch.zeros(1 << 22, dtype=torch.uint8, device=DEV)
    p = ctypes.c_void_p(buf.data_ptr())
    q = ctypes.c_void_p(buf.data_ptr() + (1 << 21))
    prm = _lib.RasterParams(P=16, M=16, sh_degree=3, W=64, H=64, tanfovx=1.0, tanfovy=1.0, scale_modifier=1.0, n_views=2,
                            per_view_appearance=1)
    assert L.d3ga_raster_preprocess(ctypes.byref(prm), p, p, None, p, None, None, p, p, p, p, p, q, 64, p, None) == -3
    assert L.d3ga_raster_preprocess_bwd(ctypes.byref(prm), p, p, None, None, p, p, p, p, q, p, p, None, p, p, None, None, None, None,
                                        None) == -3
    torch.cuda.synchronize()
