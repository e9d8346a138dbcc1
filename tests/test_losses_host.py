"""The oracle of the image losses and its case table (tests/loss_ref.py), on the CPU: the float64 maps reproduce autograd
through oracle/losses.py and the reference's own recorded values, every case exercises the seam it is there for, and a
correct float32 implementation in the device's summation order stays under the bar at every case -- before any GPU is
involved (tests/test_gpu_losses.py holds the device kernels to the same bars)."""
import functools

import numpy as np
import pytest
import torch

import loss_ref as lr
from oracle import losses as ol

f64 = torch.float64
AUTOGRAD_SHAPES = ((1, 7, 5), (3, 33, 245), (2, 17, 489))


@pytest.mark.parametrize("shape", AUTOGRAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", lr.KINDS)
def test_float64_maps_equal_autograd_of_the_oracle(kind, shape):
    a, b = lr.make_images(kind, *shape, seed=3)
    m = lr.maps(a, b, f64)
    x = a.double().requires_grad_(True)
    v = ol.ssim(x, b.double())
    (g,) = torch.autograd.grad(v, x)
    assert abs(float(m.val.mean()) - float(v.detach())) <= 1e-13
    scale = float(g.abs().max())
    if kind == "same":                                     # the gradient at the maximum is zero: its terms set the scale there
        cv = lambda t: lr._conv2d(t.abs(), lr.window2d(f64))
        scale = float((cv(m.Dm) + 2 * a.abs() * cv(m.Dq1) + b.abs() * cv(m.Dq12)).max()) / a.numel()
    err = float((m.grad_ssim - g).abs().max()) / scale
    print(f"{kind} {shape}: grad_ssim vs autograd {err:.2e} of max")
    assert err <= 1e-12
    x = a.double().requires_grad_(True)
    (g,) = torch.autograd.grad(ol.l1_loss(x, b.double()), x)
    assert torch.equal(m.grad_l1, g)
    assert abs(float((a.double() - b.double()).abs().mean()) - float(ol.l1_loss(a.double(), b.double()))) == 0.0


def test_maps_reproduce_the_reference_goldens(golden):
    g = golden("loss_cases.npz")
    for name in ("a", "b", "c"):
        pred, gt = torch.from_numpy(g[f"{name}_pred"]), torch.from_numpy(g[f"{name}_gt"])
        for dtype in (f64, torch.float32):
            m = lr.maps(pred, gt, dtype)
            assert abs(float(m.val.double().mean()) - float(g[f"{name}_ssim"])) < 2e-6
            want = g[f"{name}_ssim_grad"]
            assert float(np.abs(m.grad_ssim.numpy() - want).max()) / float(np.abs(want).max()) < 2e-5
        assert abs(float((pred.double() - gt.double()).abs().mean()) - float(g[f"{name}_l1"])) < 2e-6


def test_image_classes_are_what_they_say():
    for shape in AUTOGRAD_SHAPES + ((3, 70, 45),):
        C, H, W = shape
        a, b = lr.make_images("white", *shape, seed=1)
        assert bool((a[:, 0] == 1).all()) and bool((b[:, :, 0] == 1).all()) and bool((a[:, -1, -1] == 1).all())
        inside = a[:, H // 2 - 1: H // 2 + 2, W // 2 - 1: W // 2 + 2]
        assert float(inside.max()) <= 1.0 and float(inside.min()) < 1.0 and not torch.equal(a, b)
        a, b = lr.make_images("binary", *shape, seed=1)
        assert set(a.unique().tolist()) | set(b.unique().tolist()) <= {0.0, 1.0}
        assert bool((a[:, : H // 2] == 1).all()) and bool((b[:, : H // 2] == 1).all())
        a, b = lr.make_images("same", *shape, seed=1)
        assert torch.equal(a, b)
        a, b = lr.make_images("hdr", *shape, seed=1)
        assert float(a.max()) > 1.5 and float(a.min()) < 0.0 and 0.0 <= float(b.min()) and float(b.max()) <= 1.0
        a, b = lr.make_images("noise", *shape, seed=1)
        assert 0.0 <= float(a.min()) and float(a.max()) <= 1.0 and not torch.equal(a, b)


def _derived(c):
    """The claims of a case, from the shape and the mirrored constants alone."""
    cd = lr.ceil_div
    strips = cd(c.W, lr.MARCH_USE)
    tiles = cd(c.W, lr.TILE_W) * cd(c.H, lr.TILE_H)
    fewest_items = c.C * strips * cd(c.H, 128)
    over = [n for n, count, cap in (("tf", c.C * tiles, lr.CAP_TILED_FWD), ("mf", fewest_items, lr.CAP_MARCH_FWD),
                                    ("tb", c.C * tiles, lr.CAP_BWD), ("mb", fewest_items, lr.CAP_BWD)) if count > cap]
    rel = lambda v: "<" if c.H < v else ("=" if c.H == v else ">")
    return dict(strips=strips, last=c.W - (strips - 1) * lr.MARCH_USE, tiles=tiles, segs16=cd(c.H, lr.SEG16), w4=c.W % lr.GROUP,
                h4=c.H % lr.GROUP, hrel=rel(lr.GROUP) + rel(14) + rel(lr.SEG16), over="+".join(over) or "-")


def test_mirrored_constants_are_the_kernels():
    """loss_ref mirrors csrc/loss.hip as plain integers: read them from the source, so that the mirror cannot drift."""
    import os
    import re
    with open(os.path.join(os.path.dirname(__file__), "..", "d3ga_amd", "csrc", "loss.hip")) as f:
        src = f.read()
    k = {name: int(val) for name, val in re.findall(r"\b(k[A-Za-z0-9]+) = (\d+)\b", src)}
    assert (k["kMarchUse"], k["kSsimTW"], k["kSsimTH"]) == (lr.MARCH_USE, lr.TILE_W, lr.TILE_H)
    assert (k["kSsimTiledFwdGrid"], k["kSsimMarchFwdGrid"], k["kSsimBwdGrid"]) == (lr.CAP_TILED_FWD, lr.CAP_MARCH_FWD, lr.CAP_BWD)
    with open(os.path.join(os.path.dirname(__file__), "..", "d3ga_amd", "csrc", "d3ga_internal.h")) as f:
        assert int(re.search(r"constexpr int kBlock = (\d+);", f.read()).group(1)) == lr.L1_BLOCK
    grids = {int(v) for v in re.findall(r"loss_grid\(n4, (\d+)\)", src)}
    assert grids == {lr.L1_CAP_ATOMIC, lr.L1_CAP} and "loss_grid(n4, D3GA_LOSS_PARTIALS)" in src
    with open(os.path.join(os.path.dirname(__file__), "..", "include", "d3ga.h")) as f:
        assert int(re.search(r"#define D3GA_LOSS_PARTIALS (\d+)", f.read()).group(1)) == lr.L1_CAP
    assert "for (int rows = 16; rows <= 128; rows += 4)" in src        # seg_rows: 16 .. 128, what `over` and the seg_rows cases rest on


@pytest.mark.parametrize("case", lr.CASES, ids=lambda c: c.id)
def test_every_case_is_what_it_claims(case):
    claimed = {k: getattr(case, k) for k in ("strips", "last", "tiles", "segs16", "w4", "h4", "hrel", "over")}
    assert claimed == _derived(case)
    assert case.kind in lr.KINDS and min(case.C, case.H, case.W) >= 1
    if case.why == "cap":                                  # one segment whatever seg_rows is: the item count is C strips exactly
        assert case.H <= lr.SEG16 and case.over != "-"
    if case.why == "seg_rows":                             # two segments at the largest seg_rows; at 16 rows more items than 256 CUs x 16 workgroups
        assert case.H > 128 and case.C * case.segs16 > 4096


def test_the_table_covers_every_seam():
    noise = {(c.H, c.W) for c in lr.CASES if c.kind == "noise"}
    shapes = {(c.C, c.H, c.W) for c in lr.CASES if c.kind == "noise"}
    for W in (1, 2, 3, 4, 5, 7, 8, 11, 12, 15, 16, 17, 31, 32, 33):
        assert (9, W) in noise, W
    for W in (243, 244, 245, 248, 249, 253):
        assert (6, W) in noise, W
    for W in (488, 489, 733):
        assert (5, W) in noise, W
    for H in (1, 2, 3, 4, 5, 7, 8, 10, 11, 13, 14, 15, 16, 17, 18, 19, 20, 31, 32, 33, 63, 64, 65):
        assert (H, 6) in noise and (H, 20) in noise, H
    for s in ((2100, 3, 5), (4100, 5, 7), (8200, 3, 5), (700, 150, 6), (1500, 131, 4)):
        assert s in shapes, s
    for kind in ("white", "binary", "same", "hdr"):
        assert {(c.C, c.H, c.W) for c in lr.CASES if c.kind == kind} == {(3, 33, 245), (3, 70, 45), (1, 7, 5), (2, 17, 489)}
    small = [c for c in lr.CASES if c.kind == "noise" and c.C <= 3]
    assert {c.C for c in small} == {1, 2, 3}
    # the seams by what they are, whatever shapes provide them
    by = lambda **kw: [c for c in lr.CASES if all(getattr(c, k) == v for k, v in kw.items())]
    assert by(strips=2, last=1) and by(strips=2, last=5) and by(strips=2, last=4, w4=0) and by(strips=3) and by(strips=4)
    assert {c.h4 for c in lr.CASES if c.H <= 16} == {0, 1, 2, 3}
    assert by(hrel="=<<") and by(hrel=">=<") and by(hrel=">>=") and by(segs16=2, h4=1) and by(segs16=4, h4=0)
    assert {n for c in lr.CASES for n in c.over.split("+")} >= {"tf", "mf", "tb", "mb"}
    assert len({c.id for c in lr.CASES}) == len(lr.CASES)


@functools.lru_cache(maxsize=4)
def _oracles(case):
    a, b = lr.make_case(case)
    return lr.maps(a, b, f64), lr.maps(a, b, torch.float32), lr.maps_separable32(a, b)


@pytest.mark.parametrize("case", lr.CASES, ids=lambda c: c.id)
def test_separable_float32_stays_under_the_bar(case):
    """A correct float32 implementation in the device's order (11 + 11 taps) against the bar its 121-tap twin sets."""
    m64, m32, sep = _oracles(case)
    worst = 0.0
    for q in lr.QUANTITIES + ("grad_ssim",):
        bar = lr.bar(getattr(m64, q), getattr(m32, q))
        err = float((getattr(sep, q).double() - getattr(m64, q)).abs().max())
        worst = max(worst, err / bar)
        assert err <= bar, (q, err, bar)
    bar = lr.bar_mean_ssim(m64.val, m32.val)
    err = abs(float(sep.val.double().mean()) - float(m64.val.mean()))
    assert err <= bar, ("ssim", err, bar)
    assert torch.equal(sep.grad_l1.double(), m64.grad_l1.float().double())
    print(f"{case.id}: worst {worst:.3f} of the bar, ssim {err / bar:.3f}")
