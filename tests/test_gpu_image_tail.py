"""The image tail on the GPU (d3ga_amd/image_tail.py, csrc/image_tail.hip) against the float64 oracle of
tests/image_tail_ref.py evaluated (on the CPU, in float64) on the same float32 inputs.

Bars: the project's image bar (|a - b| <= 1e-4 on every pixel) for the forward, its element-wise gradient bar
(|a - b| <= 1e-3 |b| + 1e-6 max|b|, util.elementwise_excess) for dL/dimg, and for the camera's row of dL/dweights_raw the
same relative term plus the conditioning of its three sums (1e-6 sum |g x|: what float32 two-stage summation of C H W
products carries).  Every test prints the figure it asserts on."""
import numpy as np
import pytest
import torch

from image_tail_ref import compose_target_ref, learnable_blur_ref
from util import elementwise_excess, scene_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(4, 4), (5, 9), (64, 64), (67, 131), (747, 1022), (1080, 1920), (2160, 3840)]


def _inputs(H, W, seed, n_cam=3):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(3, H, W, generator=g), torch.randn(n_cam, 3, generator=g)


def _border(t):
    """the outermost 3 rows / columns of a (C,H,W) tensor, as a mask"""
    m = torch.zeros(t.shape[-2:], dtype=torch.bool)
    m[:3] = m[-3:] = True
    m[:, :3] = m[:, -3:] = True
    return m


@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_forward_matches_the_oracle_on_every_pixel(hw):
    from d3ga_amd.image_tail import learnable_blur
    H, W = hw
    img, wr = _inputs(H, W, seed=H * 7 + W)
    x, w = img.to(DEV), wr.to(DEV)
    cell = torch.zeros(1, dtype=torch.int32, device=DEV)
    for cam in range(wr.shape[0]):
        ref = learnable_blur_ref(img.double(), wr.double(), cam)
        out = learnable_blur(x, w, cam).cpu().double()
        cell.fill_(cam)
        assert torch.equal(learnable_blur(x, w, cell).cpu().double(), out)        # device-side index: the same launch
        d = (out - ref).abs()
        b = _border(d)
        print(f"[blur fwd] {H}x{W} cam {cam}: max |a-b| {float(d.max()):.3e}, outermost 3 rows/columns {float(d[:, b].max()):.3e}")
        assert float(d.max()) <= 1e-4
        assert float(d[:, b].max()) <= 1e-4


def _hip_grads(img, wr, cam, up):
    from d3ga_amd.image_tail import learnable_blur
    x = img.to(DEV).requires_grad_(True)
    w = wr.to(DEV).requires_grad_(True)
    out = learnable_blur(x, w, cam)
    gx, gw = torch.autograd.grad(out, [x, w], up.to(DEV))
    return out.cpu(), gx.cpu(), gw.cpu()


def _ref_grads(img, wr, cam, up):
    x = img.double().requires_grad_(True)
    w = wr.double().requires_grad_(True)
    gx, gw = torch.autograd.grad(learnable_blur_ref(x, w, cam), [x, w], up.double())
    return gx, gw


def _check_backward(img, wr, cam, up, tag):
    _, gx, gw = _hip_grads(img, wr, cam, up)
    rx, rw = _ref_grads(img, wr, cam, up)
    ex = elementwise_excess(gx.numpy(), rx.numpy())
    cond = 1e-6 * float((up.double().abs() * img.double().abs()).sum())
    allow = 1e-3 * rw[cam].abs() + cond
    ew = float(((gw[cam].double() - rw[cam]).abs() / allow).max())
    print(f"[blur bwd] {tag} cam {cam}: dL/dimg x{ex:.3f} of the element-wise bar, dL/dweights_raw[cam] x{ew:.3f} of its bar "
          f"(conditioning term {cond:.3e})")
    assert ex <= 1.0
    assert ew <= 1.0
    others = [r for r in range(wr.shape[0]) if r != cam]
    assert bool((gw[others] == 0).all()) and not bool(rw[others].any())
    return ex, ew


@pytest.mark.parametrize("hw", [(4, 4), (5, 9), (64, 64), (67, 131), (747, 1022), (1080, 1920)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_backward_matches_the_oracle_gaussian_upstream(hw):
    H, W = hw
    img, wr = _inputs(H, W, seed=H * 11 + W)
    up = torch.randn(3, H, W, generator=torch.Generator().manual_seed(H + W))
    for cam in range(wr.shape[0]):
        _check_backward(img, wr, cam, up, f"{H}x{W} gaussian g")


@pytest.mark.parametrize("hw", [(4, 4), (5, 9), (8, 4), (67, 131)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_backward_one_hot_upstream_fold_back_cases(hw):
    H, W = hw
    img, wr = _inputs(H, W, seed=H * 13 + W)
    spots = {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1),                               # corners
             (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1),                   # edges
             (1, 1), (2, 2), (3, 3), (H - 2, W - 2), (H - 3, W - 3), (H - 4, W - 4)}       # the rows / columns the ring folds onto
    for i, (y, x) in enumerate(sorted(spots)):
        up = torch.zeros(3, H, W)
        up[i % 3, y, x] = 1.0
        _check_backward(img, wr, i % wr.shape[0], up, f"{H}x{W} one-hot ({y},{x})")


@pytest.mark.parametrize("hw", [(4, 4), (5, 9), (67, 131), (747, 1022)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_adjoint_on_the_device(hw):
    """<B x, y> = <x, B^T y> with the HIP forward and the HIP backward, one blur at a time."""
    from d3ga_amd.image_tail import learnable_blur
    H, W = hw
    g = torch.Generator().manual_seed(H * 17 + W)
    x, y = torch.randn(3, H, W, generator=g), torch.randn(3, H, W, generator=g)
    for j in range(3):
        wr = torch.full((2, 3), -30.0)
        wr[1, j] = 30.0                                    # softmax -> one-hot on term j (exp(-60) vanishes against 1 in float32)
        xd = x.to(DEV).requires_grad_(True)
        Bx = learnable_blur(xd, wr.to(DEV), 1)
        (Bty,) = torch.autograd.grad(Bx, xd, y.to(DEV))
        lhs = float((Bx.detach().cpu().double() * y.double()).sum())
        rhs = float((x.double() * Bty.cpu().double()).sum())
        bound = 1e-5 * float(x.double().norm() * y.double().norm())
        print(f"[blur adjoint] {H}x{W} term {j}: |<Bx,y> - <x,B^T y>| = {abs(lhs - rhs):.3e} (bound {bound:.3e})")
        assert abs(lhs - rhs) <= bound
        if j == 0:
            assert torch.equal(Bx.detach().cpu(), x) and torch.equal(Bty.cpu(), y)         # w = (1, 0, 0): the identity


def test_hip_gradient_matches_finite_differences_of_the_hip_forward_in_weights_raw():
    """In the manner of test_known_answers.py::test_hip_backward_matches_finite_differences_of_hip_forward: central
    differences of the float32 forward along random directions (two of four aligned with the gradient, so that the relative
    bar bites), 2e-3 relative plus the rounding noise of the forward as the loss sees it."""
    from d3ga_amd.image_tail import learnable_blur
    H, W, cam = 67, 131, 1
    img, wr = _inputs(H, W, seed=5)
    x, v = img.to(DEV), wr.to(DEV)
    wts = torch.randn(3, H, W, generator=torch.Generator().manual_seed(4)).to(DEV)

    def loss(w):
        return (learnable_blur(x, w, cam).double() * wts.double()).sum()

    leaf = v.clone().requires_grad_(True)
    loss(leaf).backward()
    g = leaf.grad.double()
    with torch.no_grad():
        eps_loss = 4.0 * 6e-8 * float(((learnable_blur(x, v, cam).double() * wts.double()) ** 2).sum().sqrt())
    rng = np.random.default_rng(5)
    scale = float(v.abs().mean())
    for trial in range(4):
        d = torch.from_numpy(rng.normal(size=tuple(v.shape))).to(DEV)
        if trial < 2:
            d = d.abs() * torch.sign(g)
        h = 2e-3 * scale / float(d.abs().mean())
        with torch.no_grad():
            fd = (loss((v.double() + h * d).float()) - loss((v.double() - h * d).float())) / (2 * h)
        an = (g * d).sum()
        tol = 2e-3 * abs(float(an)) + eps_loss / h
        print(f"[blur fd] trial {trial}: fd {float(fd):.6e} analytic {float(an):.6e} tol {tol:.3e}")
        assert abs(float(fd - an)) <= tol, (trial, float(fd), float(an), tol)
        if trial < 2:
            assert eps_loss / h < 0.1 * abs(float(an)), "the aligned trials must be dominated by the relative bar"


def test_bit_identical_from_run_to_run():
    from d3ga_amd.image_tail import compose_target
    img, wr = _inputs(747, 1022, seed=3)
    up = torch.randn(3, 747, 1022, generator=torch.Generator().manual_seed(8))
    a, b = _hip_grads(img, wr, 2, up), _hip_grads(img, wr, 2, up)
    for s, t in zip(a, b):
        assert torch.equal(s, t)
    assert not bool(torch.isnan(a[2]).any()) and bool(a[2][2].any())
    x = img.to(DEV)
    args = (x, x[:1].contiguous(), x.flip(0).contiguous(), x[1:2] > 0.5, torch.rand(3, device=DEV))
    for s, t in zip(compose_target(*args), compose_target(*args)):
        assert torch.equal(s, t)


def test_small_images_and_bad_indices_are_refused():
    from d3ga_amd._lib import D3GAError
    from d3ga_amd.image_tail import LearnableBlur, learnable_blur
    w = torch.ones(2, 3, device=DEV)
    for shape in [(3, 3, 16), (3, 16, 3)]:
        with pytest.raises(D3GAError):
            learnable_blur(torch.zeros(*shape, device=DEV), w, 0)
    with pytest.raises(IndexError):
        learnable_blur(torch.zeros(3, 8, 8, device=DEV), w, 2)
    # a device-side index out of range is clamped by the kernels (nothing out of bounds is read or written)
    x = torch.rand(3, 8, 8, device=DEV)
    w = torch.randn(2, 3, device=DEV)
    hi = learnable_blur(x, w, torch.tensor([7], dtype=torch.int32, device=DEV))
    assert torch.equal(hi, learnable_blur(x, w, 1))
    lo = learnable_blur(x, w, torch.tensor([-7], dtype=torch.int32, device=DEV))
    assert torch.equal(lo, learnable_blur(x, w, 0))
    # the module: batches loop, a repeated camera receives the sum, reg is a row gather
    m = LearnableBlur(["a", "b", "c"]).to(DEV)
    with torch.no_grad():
        m.weights_raw.copy_(torch.randn(3, 3))
    xb = torch.rand(2, 3, 9, 12, device=DEV)
    up = torch.randn(2, 3, 9, 12, device=DEV)
    (gw,) = torch.autograd.grad(m(xb, ["b", "b"]), m.weights_raw, up)
    wr = m.weights_raw.detach().cpu().double().requires_grad_(True)
    ref = torch.stack([learnable_blur_ref(xb[i].cpu().double(), wr, 1) for i in range(2)])
    (rw,) = torch.autograd.grad(ref, wr, up.cpu().double())
    assert float((gw.cpu().double() - rw).abs().max()) <= 1e-3 * float(rw.abs().max()) + 1e-6 * float((up.abs() * xb.abs()).sum())
    assert bool((gw[[0, 2]] == 0).all())
    assert torch.equal(m.reg(["c", "a"]), m.weights_raw[[2, 0]])


def test_end_to_end_render_blur_loss():
    """l1_ssim(learnable_blur(render), compose_target(...)[0]).backward() reaches means3D, shs and weights_raw, and equals the
    same chain with the float64 oracle (on the CPU) in place of the two image-tail ops."""
    from d3ga_amd.image_tail import compose_target, learnable_blur
    from d3ga_amd.losses import l1_ssim
    from d3ga_amd.renderer import render
    inp = scene_inputs("T1")
    H, W = inp["H"], inp["W"]
    g = torch.Generator().manual_seed(2)
    bg = torch.rand(3, generator=g)
    frame = dict(image=torch.rand(3, H, W, generator=g), alpha=torch.rand(1, H, W, generator=g),
                 silhouette=torch.rand(3, H, W, generator=g), boundary_fg=torch.rand(1, H, W, generator=g) > 0.9)
    wr0 = torch.randn(3, 3, generator=g)
    cam = 2

    def chain(oracle):
        means = inp["means3D"].to(DEV).requires_grad_(True)
        shs = inp["shs"].to(DEV).requires_grad_(True)
        pkg = {"means3D": means, "cov3D_precomp": inp["cov6"].to(DEV), "opacities": inp["opacities"].to(DEV), "shs": shs,
               "rgb": None, "sh_degree": 3}
        img = render(inp["batch"], pkg, bg.to(DEV))["render"]
        if oracle:
            w = wr0.double().requires_grad_(True)
            gt = compose_target_ref(frame["image"].double(), frame["alpha"].double(), frame["silhouette"].double(),
                                    frame["boundary_fg"], bg.double())[0]
            pred = learnable_blur_ref(img.double().cpu(), w, cam).float().to(DEV)
            gt = gt.float().to(DEV)
        else:
            w = wr0.to(DEV).requires_grad_(True)
            gt = compose_target(frame["image"].to(DEV), frame["alpha"].to(DEV), frame["silhouette"].to(DEV),
                                frame["boundary_fg"].to(DEV), bg.to(DEV))[0]
            pred = learnable_blur(img, w, cam)
        pred.retain_grad()
        l1, ss = l1_ssim(pred, gt)
        loss = 0.8 * l1 + 0.2 * (1.0 - ss)
        loss.backward()
        cond = float((pred.grad.double().abs() * img.detach().double().abs()).sum())      # sum |g x| of the blur's three sums
        return float(loss), means.grad.cpu(), shs.grad.cpu(), w.grad.cpu(), cond

    la, ma, sa, wa, _ = chain(False)
    lb, mb, sb, wb, cond = chain(True)
    assert float(ma.abs().max()) > 0 and float(sa.abs().max()) > 0 and float(wa[cam].abs().max()) > 0
    em, es = elementwise_excess(ma.numpy(), mb.numpy()), elementwise_excess(sa.numpy(), sb.numpy())
    ew = float(((wa[cam].double() - wb[cam]).abs() / (1e-3 * wb[cam].abs() + 1e-6 * cond)).max())
    print(f"[blur e2e] loss {la:.7f} / {lb:.7f}; dL/dmeans3D x{em:.3f}, dL/dshs x{es:.3f}, dL/dweights_raw x{ew:.3f} of their bars")
    assert abs(la - lb) <= 1e-4                            # both losses are means over pixels held to the image bar
    assert em <= 1.0 and es <= 1.0 and ew <= 1.0
    assert bool((wa[[0, 1]] == 0).all())


def test_captured_step_follows_the_camera_slot():
    from d3ga_amd.graph import CapturedStep
    from d3ga_amd.image_tail import learnable_blur
    H, W = 67, 131
    img, wr = _inputs(H, W, seed=9)
    up = torch.randn(3, H, W, generator=torch.Generator().manual_seed(1))
    eager = [_hip_grads(img, wr, cam, up) for cam in range(3)]
    x = img.to(DEV).requires_grad_(True)
    w = wr.to(DEV).requires_grad_(True)
    upd = up.to(DEV)
    cell = torch.zeros(1, dtype=torch.int32, device=DEV)

    def step():
        out = learnable_blur(x, w, cell)
        (out * upd).sum().backward()
        return out, x.grad, w.grad

    cap = CapturedStep(step, params=(x, w), slots={"cam": cell})
    for cam in (0, 2, 1):
        res = cap.replay(cam=torch.tensor([cam], dtype=torch.int32))
        torch.cuda.synchronize()
        for got, want in zip(res, eager[cam]):
            assert torch.equal(got.detach().cpu(), want), cam


@pytest.mark.parametrize("kind", ["bool", "uint8", "float"])
def test_compose_target(kind):
    from d3ga_amd.image_tail import compose_target
    worst = 0.0
    for (H, W) in [(5, 9), (747, 1022), (1080, 1920)]:
        g = torch.Generator().manual_seed(H + W)
        image, alpha, sil = torch.rand(3, H, W, generator=g), torch.rand(1, H, W, generator=g), torch.rand(3, H, W, generator=g)
        bfg = torch.rand(1, H, W, generator=g) > 0.8
        if kind == "uint8":
            bfg = bfg.to(torch.uint8)
        elif kind == "float":
            bfg = bfg.float() * torch.rand(1, H, W, generator=g)          # soft masks too
        bg = torch.rand(3, generator=g)
        dev = [t.to(DEV) for t in (image, alpha, sil, bfg, bg)]
        gt, gs = compose_target(*dev)
        rt, rs = compose_target_ref(*dev)                                  # the float32 torch expression, line by line
        worst = max(worst, float((gt - rt).abs().max()), float((gs - rs).abs().max()))
        assert gt.shape == (3, H, W) and gs.shape == (3, H, W) and gt.dtype == torch.float32
        r64 = compose_target_ref(image.double(), alpha.double(), sil.double(), bfg, bg.double())
        assert float((gt.cpu().double() - r64[0]).abs().max()) <= 1e-6
    print(f"[compose_target] {kind}: max |a-b| against the float32 torch expression {worst:.3e}")
    assert worst <= 2.4e-7
