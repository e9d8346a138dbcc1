"""The image tail without a GPU: the float64 oracle (tests/image_tail_ref.py) against first principles and against the
reference's own LearnableBlur (tests/golden/blur_cases.npz, tools/gen_golden.py: gen_blur), and the new ABI surface."""
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from image_tail_ref import compose_target_ref, gaussian_blur_ref, gaussian_taps, learnable_blur_ref

NEW_EXPORTS = ("d3ga_blur_mix_fwd", "d3ga_blur_mix_bwd", "d3ga_compose_target")


def _closed_form(k):
    sigma = 0.15 * k + 0.35
    g = [math.exp(-0.5 * ((i - (k - 1) / 2) / sigma) ** 2) for i in range(k)]
    return [v / sum(g) for v in g]


@pytest.mark.parametrize("k", [3, 7])
def test_taps_sum_to_one_and_match_the_closed_form(k):
    g = gaussian_taps(k)
    assert g.dtype == torch.float64 and g.shape == (k,)
    assert abs(float(g.sum()) - 1.0) < 1e-15
    np.testing.assert_allclose(g.numpy(), _closed_form(k), rtol=1e-14, atol=0)
    assert {3: 0.8, 7: 1.4}[k] == pytest.approx(0.15 * k + 0.35, abs=1e-15)
    assert bool((g == g.flip(0)).all())


@pytest.mark.parametrize("k", [3, 7])
@pytest.mark.parametrize("hw", [(4, 4), (5, 9), (12, 7)])
def test_a_constant_image_is_a_fixed_point_also_at_the_border(k, hw):
    # with zero padding the border would come out darker (by 1 - the taps that fall outside); with reflect it does not
    img = torch.full((3, *hw), 0.37, dtype=torch.float64)
    out = gaussian_blur_ref(img, [k, k])
    assert out.shape == img.shape
    assert float((out - 0.37).abs().max()) < 1e-15


def _column(k, n, i0):
    """Hand-computed response of one axis to an impulse at i0 (n samples): the direct tap, plus the tap through the left
    reflection (output m reads input -(m + d) -> i0 when i0 >= 1: the edge sample itself is not repeated), plus the one
    through the right reflection."""
    p, g = k // 2, _closed_form(k)
    tap = lambda d: g[d + p] if -p <= d <= p else 0.0
    col = []
    for m in range(n):
        v = tap(i0 - m)
        if i0 >= 1:
            v += tap(-i0 - m)
        if i0 <= n - 2:
            v += tap(2 * (n - 1) - i0 - m)
        col.append(v)
    return col


@pytest.mark.parametrize("k", [3, 7])
def test_impulse_footprints(k):
    H, W = 11, 13
    g, p = _closed_form(k), k // 2
    # the three one-axis footprints, written out
    c0 = _column(k, H, 0)
    assert c0[:p + 1] == g[p:] and not any(c0[p + 1:])                 # impulse ON the edge: seen once, never through the mirror
    c1 = _column(k, H, 1)
    want = [2 * g[p + 1], g[p] + (g[p + 2] if p >= 2 else 0.0)]        # row 0 sees row 1 twice (directly and mirrored)
    want += [g[p + 1] + g[p + 3], g[p + 2], g[p + 3]] if k == 7 else [g[p + 1]]
    np.testing.assert_allclose(c1[:len(want)], want, rtol=1e-15)
    assert not any(c1[len(want):])
    c5 = _column(k, H, 5)
    assert c5[5 - p:5 + p + 1] == g and not any(c5[:5 - p]) and not any(c5[5 + p + 1:])
    for (y0, x0) in [(0, 0), (1, 1), (5, 6), (H - 1, W - 2), (2, W - 1)]:
        img = torch.zeros(1, H, W, dtype=torch.float64)
        img[0, y0, x0] = 1.0
        out = gaussian_blur_ref(img, [k, k])[0].numpy()
        want2 = np.outer(_column(k, H, y0), _column(k, W, x0))
        np.testing.assert_allclose(out, want2, rtol=1e-14, atol=1e-17)


def _adjoint(y, k):
    x = torch.zeros_like(y, requires_grad=True)
    (gx,) = torch.autograd.grad(gaussian_blur_ref(x, [k, k]), x, y)
    return gx


@pytest.mark.parametrize("k", [3, 7])
@pytest.mark.parametrize("hw", [(4, 4), (4, 9), (5, 6), (8, 8), (19, 23)])
def test_adjoint_identity_and_its_closed_form(k, hw):
    g = torch.Generator().manual_seed(hw[0] * 31 + hw[1] + k)
    x = torch.randn(3, *hw, generator=g, dtype=torch.float64)
    y = torch.randn(3, *hw, generator=g, dtype=torch.float64)
    Bx, Bty = gaussian_blur_ref(x, [k, k]), _adjoint(y, k)
    assert abs(float((Bx * y).sum() - (x * Bty).sum())) <= 1e-13 * float(x.norm() * y.norm())
    # the adjoint is not the blur: gradient that falls on the padded ring is folded back onto rows / columns 1..k//2
    assert float((Bty - gaussian_blur_ref(y, [k, k])).abs().max()) > 1e-3
    # ... it is the blur between two diagonal scalings, B^T = S B E: edge samples enter twice (E) and receive half (S).
    # This is what csrc/image_tail.hip computes in its backward (one tile code for both directions).
    H, W = hw
    ey = torch.ones(H, dtype=torch.float64); ey[0] = ey[-1] = 2.0
    ex = torch.ones(W, dtype=torch.float64); ex[0] = ex[-1] = 2.0
    E = ey[:, None] * ex[None, :]
    closed = gaussian_blur_ref(y * E, [k, k]) / E
    assert float((closed - Bty).abs().max()) <= 1e-14 * float(y.abs().max())


def test_oracle_equals_the_reference_module(golden):
    z = golden("blur_cases.npz")
    names = [str(s) for s in z["names"]]
    assert int(z["n"]) >= 5
    small = 0
    for i in range(int(z["n"])):
        img = torch.from_numpy(z[f"img{i}"]).requires_grad_(True)
        w = torch.from_numpy(z[f"w{i}"]).requires_grad_(True)
        idx = [names.index(str(c)) for c in z[f"cams{i}"]]
        assert idx == z[f"idx{i}"].tolist()
        assert img.dtype == torch.float64
        small += min(img.shape[-2:]) <= 8
        out = torch.stack([learnable_blur_ref(img[b], w, idx[b]) for b in range(len(idx))])
        g_img, g_w = torch.autograd.grad(out, [img, w], torch.from_numpy(z[f"up{i}"]))
        for got, name in ((out, "out"), (g_img, "g_img"), (g_w, "g_w"), (w[idx], "reg")):
            want = z[f"{name}{i}"]
            err = float(np.abs(got.detach().numpy() - want).max())
            assert err <= 1e-12 * float(np.abs(want).max()), (i, name, err)
        others = [r for r in range(len(names)) if r not in idx]
        assert not z[f"g_w{i}"][others].any() and z[f"g_w{i}"][idx].any()     # zero rows for every other camera
    assert small >= 4


def test_compose_target_ref_known_values():
    image = torch.tensor([0.2, 0.4, 0.8], dtype=torch.float64).reshape(3, 1, 1).expand(3, 1, 3).clone()
    alpha = torch.tensor([[[1.0, 0.25, 1.0]]], dtype=torch.float64)
    sil = torch.ones(3, 1, 3, dtype=torch.float64)
    bfg = torch.tensor([[[False, False, True]]])
    bg = torch.tensor([1.0, 0.0, 0.5], dtype=torch.float64)
    gt, gs = compose_target_ref(image, alpha, sil, bfg, bg)
    np.testing.assert_allclose(gt[:, 0, 0].numpy(), [0.2, 0.4, 0.8], rtol=1e-15)                     # opaque: the image
    np.testing.assert_allclose(gt[:, 0, 1].numpy(), [0.05 + 0.75, 0.1, 0.2 + 0.375], rtol=1e-15)     # blended over bg
    np.testing.assert_allclose(gt[:, 0, 2].numpy(), bg.numpy(), rtol=0)                              # boundary: background
    np.testing.assert_allclose(gs[:, 0].numpy(), [[1.0, 0.25, 0.0]] * 3, rtol=0)


def test_new_abi_surface_and_module():
    from d3ga_amd import _lib
    from d3ga_amd.image_tail import LearnableBlur, compose_target, learnable_blur        # noqa: F401
    src = open(os.path.join(ROOT, "include", "d3ga.h")).read()
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert hasattr(_lib.lib(), name)
    assert _lib.ABI_VERSION == 112 and re.search(r"#define\s+D3GA_VERSION\s+112\b", src)
    assert _lib.BLUR_PARTIALS == int(re.search(r"#define\s+D3GA_BLUR_PARTIALS\s+(\d+)", src).group(1))
    m = LearnableBlur(["a", "b"])
    sd = m.state_dict()
    assert list(sd) == ["weights_raw"] and tuple(sd["weights_raw"].shape) == (2, 3)
    assert bool((sd["weights_raw"] == 1).all()) and sd["weights_raw"].dtype == torch.float32
    assert m.name_to_idx("b").tolist() == [1] and m.name_to_idx(["b", "a"]).tolist() == [1, 0]
    assert tuple(m.reg(["b"]).shape) == (1, 3)
    m.load_state_dict({"weights_raw": torch.zeros(2, 3)}, strict=True)
    with pytest.raises(_lib.D3GAError):                                # GPU tensors only, no CPU fallback
        m(torch.zeros(1, 3, 8, 8), ["a"])
