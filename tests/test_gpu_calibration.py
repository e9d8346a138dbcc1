"""Colour calibration and pixel bias on the GPU (d3ga_amd/calibration.py, csrc/calib.hip).

Bars.  The colour forward and dL/drgb are BIT-EQUAL to the float32 torch expressions of lib/calibration.py:48-50 evaluated on
the CPU.  Every parameter gradient takes the project's element-wise gradient bar |a - b| <= 1e-3 |b| + 1e-6 max|b|
(util.elementwise_excess) against the float64 oracle of tests/calib_ref.py.  The pixel-bias forward takes
    |a - b| <= 8 eps c_max D_max + 4 eps max|bias|,   eps = 2^-24,
c_max the largest source coordinate and D_max the largest difference between adjacent map cells of the case: the first term
is a source coordinate formed in float32, the second the four-term blend.  Every test prints the figure it asserts on."""
import numpy as np
import pytest
import torch

from calib_ref import (axis_coords, color_calib_grads_ref, color_calib_ref, pixel_bias_grad_ref, pixel_bias_ref)
from util import elementwise_excess, scene_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
# the issue's sizes, plus the edges of this kernel's workgroup tile: 768 float4 = 1024 Gaussians interleaved, 3072 planar
SIZES = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 3071, 3072, 3073, 4099]
# (k, n_cameras, cameras of the views, identity camera)
BATCHES = [(1, 1, [0], None), (1, 1, [0], 0), (1, 5, [3], 1), (3, 5, [2, 1, 2], 1), (3, 5, [4, 0, 3], 1), (3, 1, [0, 0, 0], None)]
BIAS_CASES = [((8, 8), (1, 1)), ((17, 9), (1, 2)), ((40, 24), (3, 5)), ((43, 29), (3, 5)), ((72, 136), (17, 9)),
              ((9, 700), (2, 70))]            # the last: more than 32 cells and more than 256 columns per workgroup row (backward)


def _corrections(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.cat([1.0 + 0.2 * torch.randn(n, 3, generator=g), 0.1 * torch.randn(n, 3, generator=g)], 1)


def _colour_inputs(k, P, planar, seed):
    g = torch.Generator().manual_seed(seed)
    shape = (k, 3, 1, P) if planar else (k, P, 3)
    return torch.rand(*shape, generator=g), torch.randn(*shape, generator=g)


def _torch_fwd(x, cor, cams, ident, planar):
    """the float32 expression of lib/calibration.py:42-50, view by view, on the CPU"""
    out = []
    for v, c in enumerate(cams):
        w, b = cor[c, :3], cor[c, 3:]
        if c == ident:
            out.append(x[v])
        elif planar:
            out.append(x[v] * w[:, None, None] + b[:, None, None])
        else:
            out.append(x[v] * w + b)
    return torch.stack(out)


def _torch_grgb(g, cor, cams, ident, planar):
    out = []
    for v, c in enumerate(cams):
        w = cor[c, :3]
        out.append(g[v] if c == ident else (g[v] * w[:, None, None] if planar else g[v] * w))
    return torch.stack(out)


def _squeeze(t, k):
    return t[0] if k == 1 else t


@pytest.mark.parametrize("planar", [False, True], ids=["interleaved", "planar"])
@pytest.mark.parametrize("batch", BATCHES, ids=lambda b: f"k{b[0]}n{b[1]}i{b[3]}")
def test_colour_forward_and_backward(batch, planar):
    from d3ga_amd.calibration import color_calib
    k, n_cam, cams, ident = batch
    cor = _corrections(n_cam, 11 + n_cam)
    worst = 0.0
    for P in SIZES:
        x, up = _colour_inputs(k, P, planar, seed=P * 7 + k)
        xd = _squeeze(x, k).to(DEV).requires_grad_(True)
        cd = cor.to(DEV).requires_grad_(True)
        cam_arg = cams[0] if k == 1 and P % 2 else (torch.tensor(cams, dtype=torch.int32, device=DEV) if P % 3 == 0 else cams)
        out = color_calib(xd, cd, cam_arg, ident, channels_first=planar)
        gx, gc = torch.autograd.grad(out, [xd, cd], _squeeze(up, k).to(DEV))
        assert out.shape == xd.shape and out.dtype == torch.float32
        assert torch.equal(out.detach().cpu(), _squeeze(_torch_fwd(x, cor, cams, ident, planar), k)), P     # bit-equal
        assert torch.equal(gx.cpu(), _squeeze(_torch_grgb(up, cor, cams, ident, planar), k)), P             # bit-equal
        _, ref = color_calib_grads_ref(x.numpy(), cor.numpy(), cams, up.numpy(), ident, planar)
        ex = elementwise_excess(gc.cpu().numpy(), ref)
        worst = max(worst, ex)
        assert ex <= 1.0, (P, ex)
        absent = [r for r in range(n_cam) if r not in cams or r == ident]
        assert not gc[absent].any()                                    # exact zeros: cameras not in the batch, the identity row
        for c in set(cams) - {ident}:
            assert bool(gc[c].any())
    print(f"[calib] k={k} cameras={cams} identity={ident} planar={planar}: worst dL/dcorrections excess x{worst:.3f} (<= 1)")


def _hip_colour(x, cor, cams, ident, up, scale=1.0, planar=False, need=(True, True)):
    from d3ga_amd.calibration import color_calib
    xd = x.to(DEV).requires_grad_(need[0])
    cd = cor.to(DEV).requires_grad_(need[1])
    out = color_calib(xd, cd, cams, ident, grad_scale=scale, channels_first=planar)
    out.backward(up.to(DEV))
    return out.detach(), xd.grad, cd.grad


def test_colour_backward_scale_repeat_and_needs():
    cams, ident, P = [2, 1, 2], 1, 4099
    cor = _corrections(5, 3)
    x, up = _colour_inputs(3, P, False, seed=5)
    _, gx1, g1 = _hip_colour(x, cor, cams, ident, up, 1.0)
    _, gx2, g01 = _hip_colour(x, cor, cams, ident, up, 0.1)
    _, _, g1b = _hip_colour(x, cor, cams, ident, up, 1.0)
    assert torch.equal(g1, g1b) and torch.equal(gx1, gx2)              # bit-identical repeats; dL/drgb is not scaled
    _, ref = color_calib_grads_ref(x.numpy(), cor.numpy(), cams, up.numpy(), ident, grad_scale=0.1)
    ex = elementwise_excess(g01.cpu().numpy(), ref)
    ex2 = elementwise_excess(g01.cpu().numpy(), 0.1 * g1.cpu().double().numpy())
    print(f"[calib] grad_scale 0.1: excess against the oracle x{ex:.3f}, against 0.1 x the unscaled result x{ex2:.3f}")
    assert ex <= 1.0 and ex2 <= 1.0
    # one side only: the other output is None and the one asked for is unchanged
    _, gx, gc = _hip_colour(x, cor, cams, ident, up, need=(True, False))
    assert gc is None and torch.equal(gx, gx1)
    _, gx, gc = _hip_colour(x, cor, cams, ident, up, need=(False, True))
    assert gx is None and torch.equal(gc, g1)
    for planar in (False, True):
        xp, upp = _colour_inputs(2, 0, planar, seed=1)                 # P = 0 / N = 0
        out, gx, gc = _hip_colour(xp, cor, [0, 3], ident, upp, planar=planar)
        assert out.shape == xp.shape and gx.shape == xp.shape and tuple(gc.shape) == (5, 6) and not gc.any()


def _bound(bias_map, H, W):
    h, w = bias_map.shape
    c_max = max(float(axis_coords(h, H)[0].max()), float(axis_coords(w, W)[0].max()))
    d = [np.abs(np.diff(bias_map, axis=a)).max() for a in (0, 1) if bias_map.shape[a] > 1]
    d_max = float(max(d)) if d else 0.0
    return 8 * EPS * c_max * d_max, 4 * EPS * float(np.abs(bias_map).max())


@pytest.mark.parametrize("case", BIAS_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}")
@pytest.mark.parametrize("n_cam", [1, 4])
def test_pixel_bias_forward(case, n_cam):
    from d3ga_amd.calibration import pixel_bias, pixel_bias_add
    (H, W), (h, w) = case
    g = torch.Generator().manual_seed(H * 31 + W)
    bias = torch.randn(n_cam, 1, h, w, generator=g)
    bd = bias.to(DEV)
    cell = torch.zeros(1, dtype=torch.int32, device=DEV)
    for cam in range(n_cam):
        ref = pixel_bias_ref(bias[cam, 0].numpy(), H, W)
        t1, t2 = _bound(bias[cam, 0].double().numpy(), H, W)
        up = pixel_bias(bd, cam, H, W)
        assert up.shape == (1, H, W) and up.dtype == torch.float32
        err = float(np.abs(up.cpu().double().numpy()[0] - ref).max())
        print(f"[bias fwd] {H}x{W} <- {h}x{w} cam {cam}/{n_cam}: max |a-b| {err:.3e}; bound {t1:.3e} + {t2:.3e}")
        assert err <= t1 + t2
        cell.fill_(cam)
        assert torch.equal(pixel_bias(bd, cell, H, W), up)             # device-side index: the same launch
        for C in (1, 3):
            img = torch.rand(C, H, W, generator=g).to(DEV)
            assert torch.equal(pixel_bias_add(img, bd, cam), img + up)     # the fused form, bit for bit
    # a device-side index outside the table is clamped
    for bad, to in ((-3, 0), (n_cam + 5, n_cam - 1)):
        cell.fill_(bad)
        assert torch.equal(pixel_bias(bd, cell, H, W), pixel_bias(bd, to, H, W))
    with pytest.raises(IndexError):
        pixel_bias(bd, n_cam, H, W)


def _one_hots(H, W, h, w):
    """the four corners, a pixel whose source coordinate is clamped at 0 and one whose i1 is clamped at n_in - 1"""
    sy, y0, y1, _ = axis_coords(h, H)
    sx, x0, x1, _ = axis_coords(w, W)
    pts = {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)}
    low_y = np.nonzero((np.arange(H) + 0.5) * h / H - 0.5 < 0)[0]
    low_x = np.nonzero((np.arange(W) + 0.5) * w / W - 0.5 < 0)[0]
    pts.add((int(low_y[-1]), int(low_x[-1])))
    top_y, top_x = np.nonzero(y0 == h - 1)[0], np.nonzero(x0 == w - 1)[0]      # i0 == n_in - 1: i1 = i0 + 1 is clamped
    pts.add((int(top_y[0]), int(top_x[0])))
    pts.add((H // 2, W // 2))
    return sorted(pts)


@pytest.mark.parametrize("case", BIAS_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}")
def test_pixel_bias_backward(case):
    from d3ga_amd.calibration import pixel_bias, pixel_bias_add
    (H, W), (h, w) = case
    n_cam, cam = 4, 2
    g = torch.Generator().manual_seed(H * 17 + W)
    bias = torch.randn(n_cam, 1, h, w, generator=g)
    ups = [torch.randn(3, H, W, generator=g)]
    for (y, x) in _one_hots(H, W, h, w):
        e = torch.zeros(3, H, W)
        e[1, y, x] = 1.5
        ups.append(e)
    worst = 0.0
    for i, up in enumerate(ups):
        bd = bias.to(DEV).requires_grad_(True)
        img = torch.rand(3, H, W, generator=g).to(DEV).requires_grad_(True)
        out = pixel_bias_add(img, bd, cam)
        gi, gb = torch.autograd.grad(out, [img, bd], up.to(DEV))
        assert torch.equal(gi.cpu(), up)                               # dL/dimage is the upstream gradient
        ref = pixel_bias_grad_ref(up.numpy(), h, w)
        ex = elementwise_excess(gb[cam, 0].cpu().numpy(), ref)
        worst = max(worst, ex)
        assert ex <= 1.0, (i, ex)
        assert not gb[[0, 1, 3]].any()                                 # exact zeros for every other camera
        (gb2,) = torch.autograd.grad(pixel_bias_add(img, bd, cam), [bd], up.to(DEV))
        assert torch.equal(gb, gb2)                                    # bit-identical repeats
    print(f"[bias bwd] {H}x{W} <- {h}x{w}: worst excess x{worst:.3f} over a Gaussian and {len(ups) - 1} one-hot gradients")
    # the single-channel form and the adjoint identity on the device
    bd = bias.to(DEV).requires_grad_(True)
    up1 = ups[0][:1].to(DEV)
    m = pixel_bias(bd, cam, H, W)
    (gb,) = torch.autograd.grad(m, [bd], up1)
    assert elementwise_excess(gb[cam, 0].cpu().numpy(), pixel_bias_grad_ref(ups[0][:1].numpy(), h, w)) <= 1.0
    lhs = float((m.detach().double() * up1.double()).sum())
    rhs = float((bd.detach()[cam].double() * gb[cam].double()).sum())
    # both inner products are summed in float64 here; what is left is the float32 rounding of up(B) (one eps per blend step,
    # a handful of them) and of bwd(G) (one eps per term of a cell's sum), each weighted by the terms' magnitudes
    terms = float((m.detach().abs().double() * up1.abs().double()).sum())
    n_terms = 4 * (H // h + 2) * (W // w + 2)
    tol = EPS * (8 + n_terms) * terms
    print(f"[bias adjoint] {H}x{W} <- {h}x{w}: <up(B),G> - <B,bwd(G)> = {lhs - rhs:.3e}, allowed {tol:.3e}")
    assert abs(lhs - rhs) <= tol


def test_modules_reproduce_the_reference_fixture(golden):
    from d3ga_amd.calibration import CameraCalibration, CameraPixelBias
    z = golden("calib_cases.npz")
    names = [str(s) for s in z["names"]]
    for mode in ("train", "eval"):
        for i in range(int(z["n"])):
            cam = str(z[f"cam{i}"])
            m = CameraCalibration(names, str(z["identity_camera"])).to(DEV)
            m.load_state_dict({"corrections": torch.from_numpy(z[f"corr{i}"]).float()}, strict=True)
            getattr(m, mode)()
            x = torch.from_numpy(z[f"x{i}"]).float().to(DEV).requires_grad_(True)
            up = torch.from_numpy(z[f"up{i}"]).float().to(DEV)
            out = m(x, cam)
            if cam == m.identity_camera:
                assert out is x and bool(z[f"g_corr_none{i}"])
                out = out * 1.0
            gx, gc = torch.autograd.grad(out, [x, m.corrections], up, allow_unused=True)
            # the inputs are the fixture's rounded to float32 (eps each on x, w, b) and two float32 operations follow
            bar = 6 * EPS * (float(np.abs(z[f"x{i}"]).max()) * float(np.abs(z[f"corr{i}"][:, :3]).max())
                             + float(np.abs(z[f"corr{i}"][:, 3:]).max()))
            err = float(np.abs(out.detach().cpu().double().numpy() - z[f"out{i}"]).max())
            assert err <= bar, (mode, i, err, bar)
            assert elementwise_excess(gx.cpu().numpy(), z[f"g_x{i}"]) <= 1.0
            if cam == m.identity_camera:
                assert gc is None                                      # no gradient at all, not a zero one
            else:
                want = z[f"g_corr{i}"] * (1.0 if mode == "train" else 10.0)       # the fixture was recorded with the 0.1 hook
                ex = elementwise_excess(gc.cpu().numpy(), want)
                print(f"[calib module] {mode} case {i} ({cam}): out err {err:.2e} (bar {bar:.2e}), dL/dcorrections excess x{ex:.3f}")
                assert ex <= 1.0
    H, W = (int(v) for v in z["bias_hw"])
    pb = CameraPixelBias(H, W, int(z["bias_ds_rate"]), names).to(DEV)
    pb.load_state_dict({"bias": torch.from_numpy(z["bias"]).float()}, strict=True)
    idxs = z["bias_idxs"]
    out = pb(torch.from_numpy(idxs))
    assert tuple(out.shape) == z["bias_up"].shape
    (gb,) = torch.autograd.grad(out, [pb.bias], torch.from_numpy(z["bias_gout"]).float().to(DEV))
    for b, cam in enumerate(idxs.tolist()):
        t1, t2 = _bound(z["bias"][cam, 0], H, W)
        err = float(np.abs(out[b, 0].detach().cpu().double().numpy() - z["bias_up"][b, 0]).max())
        # + the fixture's parameter rounded to float32: eps max|bias| through a convex blend
        assert err <= t1 + t2 + EPS * float(np.abs(z["bias"]).max()), (b, err)
    ex = elementwise_excess(gb.cpu().numpy(), z["bias_grad"])
    print(f"[bias module] dL/dbias excess x{ex:.3f}")
    assert ex <= 1.0
    assert tuple(pb(3).shape) == (1, 1, H, W)


def _scene():
    inp = scene_inputs("T1")
    dev = {n: inp[n].to(DEV) for n in ("means3D", "cov6", "opacities", "rgb")}
    return inp, dev


def test_captured_step_follows_the_camera_slot():
    from d3ga_amd import rasterizer as R
    from d3ga_amd.calibration import color_calib, pixel_bias_add
    from d3ga_amd.graph import CapturedStep
    from d3ga_amd.losses import l1_loss
    from d3ga_amd.renderer import render
    inp, dev = _scene()
    H, W = inp["H"], inp["W"]
    n_cam, ident = 4, 1
    g = torch.Generator().manual_seed(4)
    cor = _corrections(n_cam, 8).to(DEV).requires_grad_(True)
    bias = (0.05 * torch.randn(n_cam, 1, max(W // 8, 1), max(H // 8, 1), generator=g)).to(DEV).requires_grad_(True)
    rgb = dev["rgb"].clone().requires_grad_(True)
    target = torch.rand(3, H, W, generator=g).to(DEV)
    bg = torch.ones(3, device=DEV)
    params = (rgb, cor, bias)

    def step(cam):
        pkg = {"means3D": dev["means3D"], "cov3D_precomp": dev["cov6"], "opacities": dev["opacities"], "shs": None,
               "rgb": color_calib(rgb, cor, cam, ident, grad_scale=0.1), "sh_degree": 0}
        pred = pixel_bias_add(render(inp["batch"], pkg, bg)["render"], bias, cam)
        loss = l1_loss(pred, target)
        loss.backward()
        return loss.detach(), rgb.grad, cor.grad, bias.grad

    eager = {}
    for cam in (0, 1, 3):
        for p in params:
            p.grad = None
        eager[cam] = [t.clone() for t in step(cam)]
    d = R.last_counters()["D"]
    cell = torch.zeros(1, dtype=torch.int32, device=DEV)
    R.set_capacity_policy("static", 2 * d)
    try:
        for p in params:
            p.grad = None
        cap = CapturedStep(lambda: step(cell), params=params, slots={"cam": cell})
        for cam in (3, 0, 1, 3):                                       # 1 is the identity camera
            res = cap.replay(cam=torch.tensor([cam], dtype=torch.int32))
            torch.cuda.synchronize()
            assert torch.equal(res[0], eager[cam][0]), cam             # the loss ...
            assert torch.equal(res[3], eager[cam][3]), cam             # ... and dL/dbias, which the forward alone determines
            # the colour gradients come through the rasterizer's float atomics: equal up to their summation order
            for j in (1, 2):
                assert elementwise_excess(res[j].cpu().numpy(), eager[cam][j].cpu().double().numpy()) <= 1.0, (cam, j)
    finally:
        R.set_capacity_policy("auto")
    assert not eager[1][2].any() and bool(eager[0][2][0].any())


def test_view_batched_colours_from_one_call():
    from d3ga_amd import synthetic as syn
    from d3ga_amd.calibration import color_calib
    from d3ga_amd.renderer import render, render_views
    inp, dev = _scene()
    wl = inp["scene"]["workload"]
    k, n_cam, ident, cams = 3, 5, 1, [4, 1, 4]
    batches = [syn.make_batch(wl.width, wl.height, azimuth=a) for a in (0.4, 1.3, -0.7)]
    g = torch.Generator().manual_seed(6)
    gp = torch.randn(k, 3, inp["H"], inp["W"], generator=g).to(DEV)
    bg = torch.ones(3, device=DEV)
    base = {"means3D": dev["means3D"], "cov3D_precomp": dev["cov6"], "opacities": dev["opacities"], "shs": None, "sh_degree": 0}
    rgb_views = torch.stack([dev["rgb"] * (1.0 - 0.1 * v) for v in range(k)])     # per-view colours, as a ColorField leaves them

    cor_a = _corrections(n_cam, 9).to(DEV).requires_grad_(True)
    imgs = []
    for v in range(k):
        img = render(batches[v], dict(base, rgb=color_calib(rgb_views[v], cor_a, cams[v], ident)), bg)["render"]
        (img * gp[v]).sum().backward()
        imgs.append(img.detach())
    cor_b = _corrections(n_cam, 9).to(DEV).requires_grad_(True)
    out = render_views(batches, dict(base, rgb=color_calib(rgb_views, cor_b, cams, ident)), bg)["render"]
    (out * gp).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), torch.stack(imgs))                # bit for bit
    ex = elementwise_excess(cor_b.grad.cpu().numpy(), cor_a.grad.cpu().double().numpy())
    print(f"[calib views] dL/dcorrections, one call over (3,P,3) against three calls: excess x{ex:.3f}")
    assert ex <= 1.0
    assert not cor_b.grad[[0, 1, 2, 3]].any() and bool(cor_b.grad[4].any())
