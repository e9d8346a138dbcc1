"""The VGG perceptual loss on the device (d3ga_amd/perceptual.py, csrc/perceptual.hip) against the float64 oracle of
tests/perceptual_ref.py.

Bars.  e32(q) is the float32 CPU evaluation's own max error against float64 for the same quantity q, relative to max |q|,
computed on the spot.  The device gets 4 e32: same precision, another summation order, a max statistic over a few thousand
elements.  Forward quantities: |dev - f64| <= 4 e32 max|f64|.  Gradients: |dev - f64| <= 1e-3 |f64| + f max|f64| with
f = max(1e-6, 4 e32).  Loss: sum over taps of 8 e32(tap) min(1, max|f_tap|) + 1e-6 |loss| (a tap's mean |s - t| moves by at
most the error of s plus that of t, 2 x 4 e32 max|f_tap|; where max|f_tap| > 1 the bar stays at the plain 8 e32(tap)).
Every figure is printed before it is asserted (pytest -s shows them).
"""
import pytest
import torch

import perceptual_ref as pr

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _p():
    from d3ga_amd import perceptual
    return perceptual


def _fwd_ok(name, dev, f64, f32):
    e32 = pr.e32_rel(f32, f64)
    err, m = pr.maxerr(dev.cpu(), f64), float(f64.abs().max())
    print(f"{name}: e32 {e32:.3e}  device err/max {err / max(m, 1e-300):.3e}  ratio {err / max(e32 * m, 1e-300):.2f}")
    assert err <= 4 * e32 * m, (name, err, e32, m)


def _grad_ok(name, dev, f64, f32):
    e32 = pr.e32_rel(f32, f64)
    f = max(1e-6, 4 * e32)
    x = pr.excess(dev.cpu(), f64, 1e-3, f)
    print(f"{name}: e32 {e32:.3e}  f {f:.3e}  device err/max {pr.maxerr(dev.cpu(), f64) / float(f64.abs().max()):.3e}  excess {x:.3e}")
    assert x <= 0, (name, x, e32)


# ---- 1. single operations ---------------------------------------------------------------------------------------------

WIDTHS = [(3, 64), (64, 128), (256, 256), (512, 512), (5, 33), (40, 24)]
SIZES = [(1, 1), (2, 3), (17, 18), (20, 28), (9, 15)]      # 17x18 = 306 and 9x15 = 135 pixels: no multiple of the 32 / 128 pixel tiles


@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("cc", WIDTHS, ids=lambda c: f"{c[0]}to{c[1]}")
def test_single_layer_forward_and_input_gradient(cc, hw):
    P = _p()
    (cin, cout), (H, W) = cc, hw
    g = torch.Generator().manual_seed(100 * cin + cout + H)
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = (torch.rand(cout, generator=g) - 0.5) * 0.2
    x = torch.randn(H, W, cin, generator=g)
    gy = torch.randn(H, W, cout, generator=g)
    pf, pb = P.pack_conv_weights(w.to(DEV))
    y = P.conv3x3_relu(x.to(DEV), pf, b.to(DEV), cout)
    _fwd_ok("forward", y, pr.conv3x3_relu(x.double(), w, b), pr.conv3x3_relu(x, w, b))
    # the same stored activation goes to the device and to the oracle: the masks are identical by construction
    Y = y.cpu()
    gx = P.conv3x3_relu_bwd(gy.to(DEV), y, pb, cin)
    _grad_ok("input gradient", gx, pr.conv3x3_relu_bwd(gy.double(), Y.double(), w), pr.conv3x3_relu_bwd(gy, Y, w))
    # accumulate adds to what is there
    base = torch.randn(H, W, cin, generator=g)
    acc = P.conv3x3_relu_bwd(gy.to(DEV), y, pb, cin, out=base.to(DEV), accumulate=True)
    assert torch.equal(acc, base.to(DEV) + gx)
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", [(5, 7, 5), (9, 6, 3), (2, 2, 1), (3, 3, 40), (17, 18, 33)], ids=str)
def test_pool_and_downsize_at_odd_sizes(shape):
    P = _p()
    H, W, C = shape
    g = torch.Generator().manual_seed(H * 100 + W)
    # quantised and rectified: positive ties and ties among zeros both occur
    x = torch.relu(torch.round(torch.randn(H, W, C, generator=g) * 2) / 2)
    gy = torch.randn(H // 2, W // 2, C, generator=g)
    assert torch.equal(P.maxpool2(x.to(DEV)).cpu(), pr.maxpool2(x))
    gx = P.maxpool2_bwd(x.to(DEV), gy.to(DEV)).cpu()
    assert torch.equal(gx, pr.maxpool2_bwd(x, gy))             # torch's rule: the first maximum in row-major window order
    assert not gx[2 * (H // 2):].any() and not gx[:, 2 * (W // 2):].any()      # the dropped row and column: exact zeros
    img = torch.rand(C, H, W, generator=g)
    d = P.box_down2(img.to(DEV))
    _fwd_ok("downsize", d, pr.box_down2(img.double()), pr.box_down2(img))
    gi = P.box_down2_bwd(gy.to(DEV), H, W).cpu()
    assert torch.equal(gi, pr.box_down2_bwd(gy, H, W))         # 0.25 g: exact
    assert not gi[:, 2 * (H // 2):].any() and not gi[:, :, 2 * (W // 2):].any()
    assert torch.equal(P.box_down2(img.to(DEV), down=False).cpu(), img.permute(1, 2, 0))
    assert torch.equal(P.box_down2_bwd(img.permute(1, 2, 0).contiguous().to(DEV), H, W, down=False).cpu(), img)
    torch.cuda.synchronize()


# ---- helpers of the end-to-end tests ----------------------------------------------------------------------------------

def _check_taps_and_loss(mod, pred, gt, sd, n_layers, down=True):
    """Taps and loss of one image pair against the oracle; returns (r64, r32, device loss tensor, leaf pred, leaf gt)."""
    r64 = pr.chain(pred, gt, sd, n_layers, torch.float64, down)
    r32 = pr.chain(pred, gt, sd, n_layers, torch.float32, down)
    feats = mod.features(pred.to(DEV))
    bound = 0.0
    for k, (f, a64, a32) in enumerate(zip(feats, r64["taps"], r32["taps"])):
        _fwd_ok(f"tap {k} {tuple(f.shape)}", f.permute(2, 0, 1), a64, a32)
        bound += 8 * pr.e32_rel(a32, a64) * min(1.0, float(a64.abs().max()))
    p, q = pred.to(DEV).requires_grad_(True), gt.to(DEV).requires_grad_(True)
    loss = mod(p, q)
    err, ref = abs(loss.item() - float(r64["loss"])), float(r64["loss"])
    print(f"loss {loss.item():.9g} oracle {ref:.9g} err {err:.3e} bound {bound + 1e-6 * abs(ref):.3e}")
    assert err <= bound + 1e-6 * abs(ref)
    return r64, r32, loss, p, q


def _hand_composed_gradient(P, sd, pred, gt, n_layers, down):
    """dL/dpred from the single-operation wrappers, composed by hand in the module's order, with freshly packed panels and
    every tensor in an allocation of its own."""
    nc = pr.TAPS[n_layers - 1] + 1
    pairs = [(w.to(DEV), b.to(DEV)) for w, b in pr.pairs_of(sd, nc)]
    panels = [P.pack_conv_weights(w) for w, _ in pairs]
    one = torch.ones(1, device=DEV)
    partials = torch.empty(4096, device=DEV)
    _, H, W = pred.shape
    s, t = P.box_down2(pred, down), P.box_down2(gt, down)
    acts, tap_grads, means = [], {}, []
    for i, ((w, b), (pf, _)) in enumerate(zip(pairs, panels)):
        if i in pr.POOL_BEFORE:
            s, t = P.maxpool2(s), P.maxpool2(t)
        s, t = P.conv3x3_relu(s, pf, b, w.shape[0]), P.conv3x3_relu(t, pf, b, w.shape[0])
        acts.append(s)
        if i in pr.TAPS:
            means.append(P.l1_mean(s, t, torch.empty(1, device=DEV), partials))
            tap_grads[i] = P.l1_mean_grad(s, t, one)
    loss = torch.cat(means).sum()
    g = tap_grads[nc - 1]
    for i in range(nc - 1, -1, -1):
        cin = pairs[i][0].shape[1]
        if (i - 1) in tap_grads:
            g = P.conv3x3_relu_bwd(g, acts[i], panels[i][1], cin, out=tap_grads[i - 1].clone(), accumulate=True)
        else:
            g = P.conv3x3_relu_bwd(g, acts[i], panels[i][1], cin)
        if i in pr.POOL_BEFORE:
            g = P.maxpool2_bwd(acts[i - 1], g)
    return loss, P.box_down2_bwd(g, H, W, down)


# ---- 2. full VGG19 widths ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def full_width():
    sd = pr.make_weights(pr.VGG19_WIDTHS, 0)
    P = _p()
    return sd, P.VGGLoss(5, sd).to(DEV), P.VGGLoss(5, sd, downsize=False).to(DEV)


@pytest.mark.parametrize("case", [(32, 32, True), (37, 35, True), (16, 16, False)], ids=lambda c: f"{c[0]}x{c[1]}{'' if c[2] else '-nodown'}")
def test_full_widths_end_to_end(full_width, case):
    """conv5_1 runs on 1x1 here: eight of its nine taps are padding.  The gradient is compared bit for bit with the hand
    composition of the device's own single operations (plumbing and scratch offsets at real widths); against the oracle it
    cannot be: over 20 seeds at these sizes the smallest float64 decision margin is 0-10x the layer's float32 error."""
    H, W, down = case
    sd, mod_down, mod_flat = full_width
    mod = mod_down if down else mod_flat
    pred, gt = pr.make_images(H, W, 50 + H)
    _, _, loss, p, q = _check_taps_and_loss(mod, pred, gt, sd, 5, down)
    (3.0 * loss).backward()
    assert q.grad is None
    hl, hg = _hand_composed_gradient(_p(), sd, pred.to(DEV), gt.to(DEV), 5, down)
    assert torch.equal(hl, loss.detach())
    assert torch.equal(p.grad, hg * torch.tensor(3.0, device=DEV))
    assert float(p.grad.abs().max()) > 0
    torch.cuda.synchronize()


# ---- 3. narrow chain against the oracle, qualified seeds --------------------------------------------------------------

NARROW = [(hw, s, n) for hw, seeds in pr.NARROW_SEEDS.items() for s in seeds for n in ((5, 2) if s == seeds[0] else (5,))]


@pytest.mark.parametrize("hw,seed,n_layers", NARROW, ids=lambda v: str(v).replace(" ", ""))
def test_narrow_chain_against_the_oracle(hw, seed, n_layers):
    H, W = hw
    sd = pr.make_weights(pr.NARROW_WIDTHS, seed)
    mod = _p().VGGLoss(n_layers, sd).to(DEV)
    pred, gt = pr.make_images(H, W, seed)
    r64, r32, loss, p, q = _check_taps_and_loss(mod, pred, gt, sd, n_layers)
    loss.backward()
    assert q.grad is None                                      # gt receives no gradient
    _grad_ok("dL/dpred", p.grad, r64["grad"], r32["grad"])
    torch.cuda.synchronize()


def test_narrow_chain_batch_of_two():
    (H, W), wseed, (sa, sb) = pr.NARROW_BATCH
    sd = pr.make_weights(pr.NARROW_WIDTHS, wseed)
    mod = _p().VGGLoss(5, sd).to(DEV)
    pa, pb = pr.make_images(H, W, sa), pr.make_images(H, W, sb)
    pred, gt = torch.stack([pa[0], pb[0]]), torch.stack([pa[1], pb[1]])
    r64 = [pr.chain(x, y, sd, 5, torch.float64) for x, y in (pa, pb)]
    r32 = [pr.chain(x, y, sd, 5, torch.float32) for x, y in (pa, pb)]
    p, q = pred.to(DEV).requires_grad_(True), gt.to(DEV).requires_grad_(True)
    loss = mod(p, q)
    ref = 0.5 * (float(r64[0]["loss"]) + float(r64[1]["loss"]))
    bound = max(sum(8 * pr.e32_rel(a32, a64) * min(1.0, float(a64.abs().max())) for a64, a32 in zip(r["taps"], s["taps"]))
                for r, s in zip(r64, r32))
    print(f"batch loss {loss.item():.9g} oracle {ref:.9g} bound {bound + 1e-6 * ref:.3e}")
    assert abs(loss.item() - ref) <= bound + 1e-6 * abs(ref)
    loss.backward()
    assert q.grad is None
    _grad_ok("dL/dpred (N = 2)", p.grad, 0.5 * torch.stack([r["grad"] for r in r64]), 0.5 * torch.stack([r["grad"] for r in r32]))
    torch.cuda.synchronize()


# ---- 4. the golden case ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_layers", [5, 2])
@pytest.mark.parametrize("name", ["odd", "even"])
def test_golden_case_on_the_device(golden, name, n_layers):
    """The reference's own weights and inputs (tests/golden/vgg_cases.npz): taps, loss and gradient against the oracle as in the
    narrow-chain test, and the loss the reference itself returned."""
    g = golden("vgg_cases.npz")
    sd = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w.")}
    pred, gt = torch.from_numpy(g[f"{name}_pred"]), torch.from_numpy(g[f"{name}_gt"])
    mod = _p().VGGLoss(n_layers, sd).to(DEV)
    r64, r32, loss, p, q = _check_taps_and_loss(mod, pred, gt, sd, n_layers)
    loss.backward()
    assert q.grad is None
    _grad_ok("dL/dpred", p.grad, r64["grad"], r32["grad"])
    assert abs(loss.item() - float(g[f"{name}_loss_n{n_layers}"])) <= 1e-5 * abs(loss.item())
    torch.cuda.synchronize()


# ---- 5. capture --------------------------------------------------------------------------------------------------------

def test_forward_and_backward_replay_in_a_captured_graph():
    """Forward + backward in torch.cuda.graph, replayed after a new image is written into the static input: equal to the eager
    run bit for bit, with vgg_weight * loss added to an l1_ssim term and backpropagated into the rendered image."""
    from d3ga_amd.losses import l1_ssim
    H, W, seed = 37, 53, pr.NARROW_SEEDS[(37, 53)][0]
    sd = pr.make_weights(pr.NARROW_WIDTHS, seed)
    mod = _p().VGGLoss(5, sd).to(DEV).prepare()
    first, second = pr.make_images(H, W, seed), pr.make_images(H, W, seed + 1)
    image = first[0].to(DEV).requires_grad_(True)              # the rendered image: static input of the graph
    target = first[1].to(DEV)

    def step(img, tgt):
        lv = mod(img, tgt)
        l1, s = l1_ssim(img, tgt)
        total = 0.8 * l1 + 0.2 * (1.0 - s) + 0.15 * lv
        (grad,) = torch.autograd.grad(total, img, retain_graph=True)
        (grad_v,) = torch.autograd.grad(lv, img)
        return lv.detach(), grad_v, grad, total.detach()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step(image, target)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step(image, target)
    with torch.no_grad():
        image.copy_(second[0].to(DEV))
        target.copy_(second[1].to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    eager = step(second[0].to(DEV).requires_grad_(True), second[1].to(DEV))
    assert torch.equal(captured[0], eager[0]) and torch.equal(captured[1], eager[1])      # the perceptual loss and its gradient
    assert torch.equal(captured[2], eager[2])                   # the gradient of the whole objective
    # (the objective's VALUE holds the SSIM mean, which d3ga_ssim_l1_fwd sums with float atomics: equal up to arrival order)
    assert abs(float(captured[3]) - float(eager[3])) <= 1e-6 * abs(float(eager[3]))
    assert float(captured[1].abs().max()) > 0
    # the perceptual term is in it: the gradient differs from that of the image losses alone
    img2 = second[0].to(DEV).requires_grad_(True)
    l1, s = l1_ssim(img2, second[1].to(DEV))
    (plain,) = torch.autograd.grad(0.8 * l1 + 0.2 * (1.0 - s), img2)
    assert not torch.equal(plain, eager[2]) and torch.isfinite(eager[2]).all()
    assert torch.allclose(eager[2], plain + 0.15 * eager[1], rtol=1e-5, atol=1e-9)
    torch.cuda.synchronize()
