"""The LPIPS (VGG) metric on the device (d3ga_amd/lpips.py, csrc/lpips.hip, the batched entry points of csrc/perceptual.hip)
against the float64 restatement of tests/lpips_ref.py (parity with the `lpips` package itself is unpinned: DESIGN.md 4.4i).

Bars, by the rule of test_gpu_perceptual.py.  e32(q) is the float32 CPU oracle's max error against float64 for the same
quantity q, relative to max |q|, computed on the spot and printed.  Maps, features and the scaled input: |dev - f64| <= 4 e32
max|f64|.  The metric value: sum over taps of 4 e32(map_t) max|map_t| (a mean moves by no more than its terms), plus 1e-6
|value|.  Whatever is stated to be bit-identical (a batch against single calls, a replay against eager, a == b -> 0, the
one-hot answers) is held with torch.equal / ==.  Every figure is printed before it is asserted (pytest -s shows them)."""
import pytest
import torch

import lpips_ref as lr
import perceptual_ref as pr

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _m():
    from d3ga_amd import lpips
    return lpips


def _fwd_ok(name, dev, f64, f32):
    e32 = lr.e32_rel(f32, f64)
    err, m = lr.maxerr(dev.cpu(), f64), float(f64.abs().max())
    print(f"{name}: e32 {e32:.3e}  device err/max {err / max(m, 1e-300):.3e}  ratio {err / max(e32 * m, 1e-300):.2f}")
    assert err <= 4 * e32 * m, (name, err, e32, m)
    return 4 * e32 * m


# ---- 1. batched convolution and pool ------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("hw", [(17, 18), (9, 15), (1, 1)], ids=lambda s: f"{s[0]}x{s[1]}")      # 306 and 135 pixels: a wavefront straddles the seam
@pytest.mark.parametrize("cc", [(3, 64), (5, 33), (64, 128)], ids=lambda c: f"{c[0]}to{c[1]}")
def test_batched_conv_and_pool_equal_the_single_image_calls(cc, hw, N):
    from d3ga_amd import perceptual as P
    (cin, cout), (H, W) = cc, hw
    g = torch.Generator().manual_seed(1000 * cin + 10 * cout + H + N)
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = ((torch.rand(cout, generator=g) - 0.5) * 0.2).to(DEV)
    x = torch.randn(N, H, W, cin, generator=g).to(DEV)
    gy = torch.randn(N, H, W, cout, generator=g).to(DEV)
    base = torch.randn(N, H, W, cin, generator=g).to(DEV)
    pf, pb = P.pack_conv_weights(w.to(DEV))
    one = lambda t, n: t[n].clone()                             # an allocation of its own: 16-byte aligned whatever H W C is
    # forward, no mask
    y = P.conv3x3_n(x, pf, b, cout)
    singles = [P.conv3x3_relu(one(x, n), pf, b, cout) for n in range(N)]
    assert all(torch.equal(y[n], singles[n]) for n in range(N))
    assert float(y.abs().max()) > 0
    # the seam is real: the batch as ONE tall image differs where rows of two images would touch
    if H > 1:
        tall = P.conv3x3_relu(x.view(N * H, W, cin), pf, b, cout).view(N, H, W, cout)
        assert not torch.equal(tall[0, H - 1], y[0, H - 1]) and torch.equal(tall[0, :H - 1], y[0, :H - 1])
    # and it is the oracle's convolution, image by image
    _fwd_ok("batched forward", y[N - 1], pr.conv3x3_relu(x[N - 1].cpu().double(), w, b.cpu()), pr.conv3x3_relu(x[N - 1].cpu(), w, b.cpu()))
    # forward with accumulate
    acc = P.conv3x3_n(x, pf, b, cout, out=gy.clone(), accumulate=True)
    for n in range(N):
        xn, s = one(x, n), one(gy, n)
        st = P._lib.lib().d3ga_vgg_conv3x3(H, W, cin, cout, P.dptr(xn), None, P.dptr(pf), P.dptr(b), 1, 1, P.dptr(s), P.stream_handle())
        assert st == 0 and torch.equal(acc[n], s)
    # the input-gradient form: mask_y, transposed panel, no bias, no ReLU -- alone and accumulating
    gx = P.conv3x3_n(gy, pb, None, cin, relu=False, mask_y=y)
    gacc = P.conv3x3_n(gy, pb, None, cin, relu=False, mask_y=y, out=base.clone(), accumulate=True)
    for n in range(N):
        assert torch.equal(gx[n], P.conv3x3_relu_bwd(one(gy, n), singles[n], pb, cin))
        assert torch.equal(gacc[n], P.conv3x3_relu_bwd(one(gy, n), singles[n], pb, cin, out=one(base, n), accumulate=True))
    # the pool: quantised and rectified input, so that ties occur
    if H >= 2:
        q = torch.relu(torch.round(x * 2) / 2)
        p = P.maxpool2_n(q)
        assert tuple(p.shape) == (N, H // 2, W // 2, cin)
        for n in range(N):
            assert torch.equal(p[n], P.maxpool2(one(q, n))) and torch.equal(p[n].cpu(), pr.maxpool2(q[n].cpu()))
    torch.cuda.synchronize()


# ---- 2. the input layer ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("hw", [(1, 1), (5, 7)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_input_layer(hw, N, normalize):
    H, W = hw
    img = torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(H + N))
    out = _m().scale_input(img.to(DEV), normalize)
    assert tuple(out.shape) == (N, H, W, 3)
    _fwd_ok("scaled input", out.permute(0, 3, 1, 2), lr.scale_input(img.double(), normalize), lr.scale_input(img, normalize))
    assert not torch.equal(out, _m().scale_input(img.to(DEV), not normalize))
    torch.cuda.synchronize()


# ---- 3. the tap distance alone --------------------------------------------------------------------------------------------

TAP_SIZES = ((1, 1), (2, 3), (17, 18))


def _tap_inputs(B, h, w, C, g):
    """Rectified features (zeros occur, as behind a ReLU), pixel 0 zeroed on one side and, where there is one, pixel 1 on both;
    weights in [0, 0.2) with one negative entry."""
    a, b = torch.relu(torch.randn(B, h, w, C, generator=g) + 0.5), torch.relu(torch.randn(B, h, w, C, generator=g) + 0.5)
    a.view(B, h * w, C)[:, 0] = 0
    if h * w > 1:
        a.view(B, h * w, C)[:, 1] = 0
        b.view(B, h * w, C)[:, 1] = 0
    lin = torch.rand(C, generator=g) * 0.2
    lin[C // 2] = -0.05
    return a, b, lin


def _oracle_map(a, b, lin, dtype):
    return lr.tap_distance(a.to(dtype).permute(0, 3, 1, 2), b.to(dtype).permute(0, 3, 1, 2), lin)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C", [1, 8, 20, 33, 64, 512])
def test_tap_distance(C, B):
    """Every (h, w) of TAP_SIZES for one (C, B).  q of the bar is the three sizes' maps together (313 B pixels): e32 is a max
    statistic, and over the single pixel of a 1 x 1 map it would measure nothing."""
    L = _m()
    g = torch.Generator().manual_seed(100 * C + B)
    dev_maps, m64, m32, values = [], [], [], []
    for h, w in TAP_SIZES:
        a, b, lin = _tap_inputs(B, h, w, C, g)
        A, Bt, LIN = a.to(DEV), b.to(DEV), lin.to(DEV)
        value, m = L.tap_distance(A, Bt, LIN)
        assert tuple(m.shape) == (B, h, w) and tuple(value.shape) == (B,)
        assert bool(torch.isfinite(m).all())                      # the zeroed pixels: no NaN
        if h * w > 1:
            assert not m.view(B, -1)[:, 1].any()                  # both sides zero: exactly 0
        # a batch is bit for bit its single-pair calls; no map asked for: the same value; accumulate adds to the cell
        for i in range(B):
            vi, mi = L.tap_distance(A[i:i + 1].clone(), Bt[i:i + 1].clone(), LIN)
            assert torch.equal(mi[0], m[i]) and torch.equal(vi[0], value[i])
        v2, none = L.tap_distance(A, Bt, LIN, want_map=False)
        assert none is None and torch.equal(v2, value)
        v3, _ = L.tap_distance(A, Bt, LIN, want_map=False, value=value.clone(), accumulate=True)
        assert torch.equal(v3, value + value)
        # a == b: exactly zero, map and value
        vz, mz = L.tap_distance(A, A, LIN)
        assert not mz.any() and not vz.any()
        o64, o32 = _oracle_map(a, b, lin, torch.float64), _oracle_map(a, b, lin, torch.float32)
        dev_maps.append(m.cpu().reshape(-1)); m64.append(o64.reshape(-1)); m32.append(o32.reshape(-1))
        values.append((value.cpu(), o64.mean(dim=(1, 2))))
    bar = _fwd_ok(f"maps C={C} B={B}", torch.cat(dev_maps), torch.cat(m64), torch.cat(m32))
    for (h, w), (v, v64) in zip(TAP_SIZES, values):
        err = float((v.double() - v64).abs().max())
        print(f"  value {h}x{w}: err {err:.3e} bound {bar + 1e-6 * float(v64.abs().max()):.3e}")
        assert err <= bar + 1e-6 * float(v64.abs().max())
    torch.cuda.synchronize()


@pytest.mark.parametrize("C", [2, 8, 20, 33, 64, 512])
def test_tap_distance_known_answers(C):
    """First-principles answers, independent of any recall of the package; exact where they are exact."""
    L = _m()
    g = torch.Generator().manual_seed(C)
    lin = torch.rand(C, generator=g) * 0.2
    lin[C // 2] = -0.05
    pairs = [(0, C - 1), (C - 1, 0), (C // 2, 0), (1, C // 2), (C // 3, C - 1 - C // 3)]
    pairs = [(i, j) for i, j in pairs if i != j]
    P = len(pairs)
    eye = torch.eye(C)
    a = torch.stack([eye[i] for i, _ in pairs]).view(1, 1, P, C)
    b = torch.stack([eye[j] for _, j in pairs]).view(1, 1, P, C)
    LIN = lin.to(DEV)
    _, m = L.tap_distance(a.to(DEV), b.to(DEV), LIN)
    want = torch.stack([lin[i] + lin[j] for i, j in pairs])
    print("one-hot", m.cpu().view(-1).tolist(), want.tolist())
    assert torch.equal(m.cpu().view(-1), want)                                       # a = e_i, b = e_j: lin_i + lin_j
    v, m0 = L.tap_distance(torch.zeros_like(a).to(DEV), b.to(DEV), LIN)
    assert torch.equal(m0.cpu().view(-1), torch.stack([lin[j] for _, j in pairs]))   # a = 0, b = e_j: lin_j
    _, m1 = L.tap_distance(b.to(DEV), torch.zeros_like(a).to(DEV), LIN)
    assert torch.equal(m1, m0)
    # d(alpha a, beta b) = d(a, b): powers of two exactly (entries in [0.5, 2.5): 1e-10 is far below half an ulp of the norms)
    x, y = (torch.rand(1, 5, 7, C, generator=g) * 2 + 0.5), (torch.rand(1, 5, 7, C, generator=g) * 2 + 0.5)
    _, d = L.tap_distance(x.to(DEV), y.to(DEV), LIN)
    _, d2 = L.tap_distance((4 * x).to(DEV), (0.5 * y).to(DEV), LIN)
    assert torch.equal(d, d2)
    # any positive factors: the float64 oracle is invariant (to the 1e-10 it adds to the norms), the device meets it under the bar
    xs, ys = 3.7 * x, 0.31 * y
    _, d3 = L.tap_distance(xs.to(DEV), ys.to(DEV), LIN)
    o64, s64 = _oracle_map(x, y, lin, torch.float64), _oracle_map(xs, ys, lin, torch.float64)
    exact = _oracle_map(3.7 * x.double(), 0.31 * y.double(), lin, torch.float64)       # scaled in double: xs, ys carry a float32 rounding
    assert float((o64 - exact).abs().max()) <= 1e-8 * float(o64.abs().max())
    _fwd_ok("d(a, b)", d, o64, _oracle_map(x, y, lin, torch.float32))
    _fwd_ok("d(3.7 a, 0.31 b)", d3, s64, _oracle_map(xs, ys, lin, torch.float32))
    torch.cuda.synchronize()


# ---- 4. - 6. the chain ----------------------------------------------------------------------------------------------------

def _check_chain(mod, fake, target, sd, normalize):
    """One pair (3,H,W) against the oracle: five maps and the value."""
    r64 = lr.chain(fake[None], target[None], sd, normalize)
    r32 = lr.chain(fake[None], target[None], sd, normalize, torch.float32)
    F, T = fake.to(DEV), target.to(DEV)
    maps = mod.maps(F, T)
    assert [tuple(m.shape) for m in maps] == [tuple(m.shape[1:]) for m in r64["maps"]]
    bound = 0.0
    for k, (m, a64, a32) in enumerate(zip(maps, r64["maps"], r32["maps"])):
        bound += _fwd_ok(f"map {k} {tuple(m.shape)}", m, a64[0], a32[0])
    out = mod(F, T)
    assert tuple(out.shape) == (1, 1, 1, 1) and out.dtype == torch.float32 and not out.requires_grad
    v, ref = float(out), float(r64["value"])
    print(f"value {v:.9g} oracle {ref:.9g} err {abs(v - ref):.3e} bound {bound + 1e-6 * abs(ref):.3e}")
    assert abs(v - ref) <= bound + 1e-6 * abs(ref)
    assert not float(mod(F, F))                                 # d(x, x) == 0 through the whole chain
    return out


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("hw", lr.NARROW_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_narrow_chain_against_the_oracle(hw, normalize):
    H, W = hw
    for seed in lr.NARROW_SEEDS[hw][normalize]:
        sd = lr.make_weights(pr.NARROW_WIDTHS, seed, "package" if seed % 2 else "torchvision", "lins" if seed % 2 else "lin")
        mod = _m().LPIPS("vgg", sd, normalize=normalize).to(DEV)
        fake, target = pr.make_images(H, W, seed)
        _check_chain(mod, fake, target, sd, normalize)
    torch.cuda.synchronize()


def test_true_vgg16_widths():
    (H, W), seed = lr.VGG16_CASE
    sd = lr.make_weights(lr.VGG16_WIDTHS, seed)
    mod = _m().LPIPS("vgg", sd).cuda()
    assert mod.widths == lr.VGG16_WIDTHS
    fake, target = pr.make_images(H, W, seed)
    _check_chain(mod, fake, target, sd, False)
    torch.cuda.synchronize()


def test_batch_of_two_is_bit_identical_to_two_single_calls():
    H, W, seed = 37, 53, lr.NARROW_SEEDS[(37, 53)][False][0]
    sd = lr.make_weights(pr.NARROW_WIDTHS, seed)
    mod = _m().LPIPS("vgg", sd).to(DEV)
    fake, target = (t.to(DEV) for t in pr.make_images(H, W, seed, n=2))
    out = mod(fake, target)
    maps = mod.maps(fake, target)
    assert tuple(out.shape) == (2, 1, 1, 1) and [tuple(m.shape) for m in maps] == [(2, 37, 53), (2, 18, 26), (2, 9, 13), (2, 4, 6), (2, 2, 3)]
    for i in range(2):
        single = mod(fake[i], target[i])
        assert tuple(single.shape) == (1, 1, 1, 1) and torch.equal(single[0], out[i])
        assert all(torch.equal(s, m[i]) for s, m in zip(mod.maps(fake[i], target[i]), maps))
        assert torch.equal(mod(fake[i:i + 1], target[i:i + 1]), single)
    assert float(out[0]) != float(out[1])
    r64 = lr.chain(fake.cpu(), target.cpu(), sd)
    assert torch.allclose(out.view(2).cpu().double(), r64["value"], rtol=1e-4, atol=0)
    torch.cuda.synchronize()


# ---- 7. capture -------------------------------------------------------------------------------------------------------------

def test_replay_of_a_captured_call_is_bit_identical_to_eager():
    H, W, seed = 37, 53, lr.NARROW_SEEDS[(37, 53)][False][1]
    sd = lr.make_weights(pr.NARROW_WIDTHS, seed)
    mod = _m().LPIPS("vgg", sd).to(DEV).prepare(H, W, 2)
    first, second = pr.make_images(H, W, seed, n=2), pr.make_images(H, W, seed + 5, n=2)
    fake, target = first[0].to(DEV), first[1].to(DEV)          # the static inputs of the graph
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            mod(fake, target)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = mod(fake, target)
    fake.copy_(second[0].to(DEV))
    target.copy_(second[1].to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    got = captured.clone()
    eager = mod(second[0].to(DEV), second[1].to(DEV))
    print("replay", got.view(-1).tolist(), "eager", eager.view(-1).tolist())
    assert torch.equal(got, eager) and float(eager.abs().min()) > 0
    assert not torch.equal(eager, mod(first[0].to(DEV), first[1].to(DEV)))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, eager)
    torch.cuda.synchronize()


# ---- 8. the evaluation line -------------------------------------------------------------------------------------------------

def test_evaluator_takes_the_module(tmp_path):
    from d3ga_amd import Evaluator, compute_errors
    H, W, seed = 37, 53, 0
    sd = lr.make_weights(pr.NARROW_WIDTHS, seed)
    mod = _m().LPIPS("vgg", sd).cuda()
    g = torch.Generator().manual_seed(7)
    ev = Evaluator("white", lpips=mod)
    values = []
    for B in (None, 2):                                         # one frame, then a batch of two
        shape = (3, H, W) if B is None else (B, 3, H, W)
        pred, image = torch.rand(shape, generator=g).to(DEV), torch.rand(shape, generator=g).to(DEV)
        alpha = torch.rand(shape[:-3] + (1, H, W), generator=g).to(DEV)
        boundary = (torch.rand(shape[:-3] + (1, H, W), generator=g) > 0.9).to(DEV)
        out = ev.add(pred, image, alpha, boundary)
        if B is None:
            assert out["lpips"].dim() == 0 and torch.equal(out["lpips"], mod(pred, out["target"]).mean())
            values.append(float(out["lpips"]))
            heat, s, p, l = compute_errors(out["target"], pred, lpips=mod)
            assert l == float(out["lpips"])
        else:
            assert tuple(out["lpips"].shape) == (B,)
            assert torch.equal(out["lpips"], mod(pred, out["target"]).view(B))       # per frame there, one batch here: the same bits
            values += out["lpips"].tolist()
    m = ev.summary()
    assert m["count"] == 3 and m["lpips"] == pytest.approx(sum(values) / 3, rel=1e-12) and m["lpips"] > 0
    path = tmp_path / "errors_cam_test.txt"
    ev.write(str(path))
    line = path.read_text()
    print(line.strip())
    assert line == f"SSIM: {m['ssim']:.5f}, PSNR: {m['psnr']:.5f}, LPIPS: {m['lpips']:.5f}\n" and "nan" not in line
    torch.cuda.synchronize()
