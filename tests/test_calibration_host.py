"""Colour calibration and pixel bias without a GPU: the float64 oracle (tests/calib_ref.py) against the reference's own
CameraCalibration / CameraPixelBias (tests/golden/calib_cases.npz, tools/gen_golden.py: gen_calib) and against first
principles (rows of U, the adjoint identity, the contiguous cell ranges), the new ABI surface and its refusals, and the two
modules' state dicts."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from calib_ref import (axis_coords, cell_ranges, color_calib_grads_ref, color_calib_ref, interp_matrix, pixel_bias_grad_ref,
                       pixel_bias_ref)
from conftest import ROOT

NEW_EXPORTS = ("d3ga_color_calib_fwd", "d3ga_color_calib_bwd", "d3ga_pixel_bias_fwd", "d3ga_pixel_bias_bwd")
E_NULL, E_SIZE, E_CONFIG = -1, -2, -3            # D3GA_E_* (include/d3ga.h)
MAPS = [((1, 1), (40, 24)), ((1, 2), (40, 24)), ((3, 5), (40, 24)), ((3, 5), (43, 29))]


def _close(got, want, what):
    err = float(np.abs(np.asarray(got) - want).max())
    assert err <= 1e-12 * max(float(np.abs(want).max()), 1e-300), (what, err)


def test_oracle_equals_the_reference_calibration(golden):
    z = golden("calib_cases.npz")
    names = [str(s) for s in z["names"]]
    ident = names.index(str(z["identity_camera"]))
    seen = set()
    for i in range(int(z["n"])):
        kind, cam = str(z[f"kind{i}"]), names.index(str(z[f"cam{i}"]))
        cf = kind == "img"
        x, corr, up = z[f"x{i}"], z[f"corr{i}"], z[f"up{i}"]
        assert x.dtype == np.float64
        seen.add((kind, cam == ident))
        _close(color_calib_ref(x[None], corr, [cam], ident, cf)[0], z[f"out{i}"], (i, "out"))
        g_x, g_c = color_calib_grads_ref(x[None], corr, [cam], up[None], ident, cf, grad_scale=0.1)      # training mode: the hook
        _close(g_x[0], z[f"g_x{i}"], (i, "g_x"))
        if cam == ident:                                      # the reference returns its input: no gradient at all
            assert bool(z[f"g_corr_none{i}"]) and not g_c.any()
            assert np.array_equal(z[f"out{i}"], x) and np.array_equal(z[f"g_x{i}"], up)
        else:
            assert not bool(z[f"g_corr_none{i}"])
            _close(g_c, z[f"g_corr{i}"], (i, "g_corr"))
            others = [r for r in range(len(names)) if r != cam]
            assert not z[f"g_corr{i}"][others].any() and z[f"g_corr{i}"][cam].all()
            # the hook scales the parameter gradient alone: without it the oracle is ten times the golden
            _close(0.1 * color_calib_grads_ref(x[None], corr, [cam], up[None], ident, cf)[1], z[f"g_corr{i}"], (i, "scale"))
    assert seen == {("pts", False), ("pts", True), ("img", False), ("img", True)}


def test_oracle_equals_the_reference_pixel_bias(golden):
    z = golden("calib_cases.npz")
    H, W = (int(v) for v in z["bias_hw"])
    bias, idxs = z["bias"], z["bias_idxs"].tolist()
    assert bias.shape == (4, 1, W // 8, H // 8)               # the reference's swapped sizes
    want = np.zeros_like(bias)
    for b, cam in enumerate(idxs):
        _close(pixel_bias_ref(bias[cam, 0], H, W), z["bias_up"][b, 0], ("up", b))
        want[cam, 0] += pixel_bias_grad_ref(z["bias_gout"][b], bias.shape[2], bias.shape[3])
    _close(want, z["bias_grad"], "bias_grad")
    others = [r for r in range(bias.shape[0]) if r not in idxs]
    assert not z["bias_grad"][others].any()


@pytest.mark.parametrize("n_in,n_out", [(1, 8), (2, 9), (3, 40), (5, 24), (3, 43), (5, 29), (93, 1022), (127, 747), (9, 4)])
def test_interpolation_rows_sum_to_one_and_ranges_are_contiguous(n_in, n_out):
    U = interp_matrix(n_in, n_out)
    assert float(np.abs(U.sum(1) - 1.0).max()) <= 4e-16
    assert U.min() >= 0.0
    src, i0, i1, lam = axis_coords(n_in, n_out)
    assert (np.diff(i0) >= 0).all() and (lam >= 0).all() and src[0] == max(0.0, 0.5 * n_in / n_out - 0.5)
    R = cell_ranges(n_in, n_out)
    for i in range(n_in):
        touched = np.nonzero(U[:, i])[0]
        lo, hi = R[i]
        if len(touched):
            assert (np.diff(touched) == 1).all()              # one contiguous run ...
            assert lo <= touched[0] and touched[-1] < hi      # ... inside the range the kernel walks
        assert ((i0[lo:hi] == i) | (i0[lo:hi] == i - 1)).all()
        assert not ((i0[:lo] == i) | (i1[:lo] == i)).any() and not ((i0[hi:] == i) | (i1[hi:] == i)).any()
    # neighbouring cells share exactly the pixels that sit between them: those with i0 == i
    for i in range(n_in - 1):
        shared = set(range(R[i][0], R[i][1])) & set(range(R[i + 1][0], R[i + 1][1]))
        assert shared == set(np.nonzero(i0 == i)[0].tolist())
    # cells two apart share nothing
    for i in range(n_in - 2):
        assert R[i][1] <= R[i + 2][0]


@pytest.mark.parametrize("hw,HW", MAPS, ids=lambda v: "x".join(map(str, v)))
def test_adjoint_identity(hw, HW):
    rng = np.random.default_rng(hw[0] * 100 + HW[0])
    B, G = rng.normal(size=hw), rng.normal(size=HW)
    lhs = float((pixel_bias_ref(B, *HW) * G).sum())
    rhs = float((B * pixel_bias_grad_ref(G, *hw)).sum())
    scale = float(np.abs(pixel_bias_ref(B, *HW) * G).sum())
    assert abs(lhs - rhs) <= 1e-14 * scale
    G3 = rng.normal(size=(3,) + HW)                           # the fused form: the gradient of a broadcast sums the channels
    np.testing.assert_allclose(pixel_bias_grad_ref(G3, *hw), sum(pixel_bias_grad_ref(G3[c], *hw) for c in range(3)), rtol=1e-13,
                               atol=1e-13)


def test_oracle_matches_interpolate_in_float64():
    import torch.nn.functional as F
    for hw, HW in MAPS:
        B = torch.randn(1, 1, *hw, dtype=torch.float64, generator=torch.Generator().manual_seed(hw[1]), requires_grad=True)
        up = F.interpolate(B, size=HW, mode="bilinear")
        G = torch.randn(up.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
        (gB,) = torch.autograd.grad(up, [B], G)
        _close(pixel_bias_ref(B.detach().numpy()[0, 0], *HW), up.detach().numpy()[0, 0], "up")
        _close(pixel_bias_grad_ref(G.numpy()[0], *hw), gB.numpy()[0, 0], "grad")


def test_new_abi_surface():
    from d3ga_amd import _lib
    src = open(os.path.join(ROOT, "include", "d3ga.h")).read()
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert hasattr(_lib.lib(), name)
    assert _lib.ABI_VERSION == 112 and re.search(r"#define\s+D3GA_VERSION\s+112\b", src)
    assert _lib.lib().d3ga_version() == 112
    assert _lib.CALIB_PARTIALS == int(re.search(r"#define\s+D3GA_CALIB_PARTIALS\s+(\d+)", src).group(1))
    assert "calib.hip" in open(os.path.join(ROOT, "d3ga_amd", "csrc", "build.py")).read()


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """The refusals happen before any HIP call: host buffers stand in for device memory and are never touched."""
    from d3ga_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)   # 16-byte aligned
    odd = ctypes.c_void_p(p.value + 4)
    # colour forward: (k, n, planar, n_cameras, identity_idx, rgb, corrections, cam, out, stream)
    fwd = L.d3ga_color_calib_fwd
    assert fwd(0, 4, 0, 2, 0, p, p, p, p, None) == E_SIZE
    assert fwd(1, -1, 0, 2, 0, p, p, p, p, None) == E_SIZE
    assert fwd(1, 4, 0, 0, -1, p, p, p, p, None) == E_SIZE
    assert fwd(1, 4, 0, 2, 2, p, p, p, p, None) == E_SIZE                     # identity_idx outside the table
    assert fwd(_lib.CALIB_PARTIALS, 4, 0, 2, 0, p, p, p, p, None) == E_SIZE   # more views than rows of partials
    assert fwd(1, 2 ** 30, 0, 2, 0, p, p, p, p, None) == E_SIZE               # 3 k n past INT32_MAX
    assert fwd(1, 4, 2, 2, 0, p, p, p, p, None) == E_CONFIG
    for bad in range(4):
        args = [p, p, p, p]
        args[bad] = None
        assert fwd(1, 4, 0, 2, 0, *args, None) == E_NULL, bad
    assert fwd(1, 4, 0, 2, 0, odd, p, p, p, None) == E_CONFIG and fwd(1, 4, 1, 2, 0, p, p, p, odd, None) == E_CONFIG
    assert fwd(3, 0, 0, 2, 0, None, p, p, None, None) == 0                    # n == 0: valid, nothing to launch
    # colour backward: (k, n, planar, n_cameras, identity_idx, grad_scale, rgb, corrections, cam, grad_out, grad_rgb,
    #                   grad_corrections, partials, stream)
    bwd = L.d3ga_color_calib_bwd
    assert bwd(0, 4, 0, 2, 0, 1.0, p, p, p, p, p, p, p, None) == E_SIZE
    assert bwd(1, -4, 1, 2, 0, 1.0, p, p, p, p, p, p, p, None) == E_SIZE
    assert bwd(1, 4, 0, -1, 0, 1.0, p, p, p, p, p, p, p, None) == E_SIZE
    assert bwd(1, 4, 0, 2, 0, 1.0, p, None, p, p, p, p, p, None) == E_NULL    # corrections
    assert bwd(1, 4, 0, 2, 0, 1.0, p, p, None, p, p, p, p, None) == E_NULL    # cam
    assert bwd(1, 4, 0, 2, 0, 1.0, p, p, p, None, p, p, p, None) == E_NULL    # grad_out
    assert bwd(1, 4, 0, 2, 0, 1.0, p, p, p, p, None, None, p, None) == E_NULL  # no output at all
    assert bwd(1, 4, 0, 2, 0, 1.0, None, p, p, p, p, p, p, None) == E_NULL    # grad_corrections needs rgb ...
    assert bwd(1, 4, 0, 2, 0, 1.0, p, p, p, p, p, p, None, None) == E_NULL    # ... and the scratch
    assert bwd(1, 4, 0, 2, 0, 1.0, p, p, p, odd, p, p, p, None) == E_CONFIG
    assert bwd(2, 0, 0, 2, 0, 1.0, None, p, p, None, None, None, None, None) == 0      # n == 0 and no parameter gradient
    # pixel bias forward: (C, H, W, n_cameras, bh, bw, bias, cam, image, out, stream)
    pf = L.d3ga_pixel_bias_fwd
    for bad in range(6):
        sizes = [3, 8, 8, 2, 1, 1]
        sizes[bad] = 0
        assert pf(*sizes, p, p, p, p, None) == E_SIZE, bad
        sizes[bad] = -3
        assert pf(*sizes, p, p, None, p, None) == E_SIZE, bad
    assert pf(3, 2 ** 15, 2 ** 15, 2, 1, 1, p, p, p, p, None) == E_SIZE
    assert pf(1, 2 ** 16, 8, 1, 2 ** 14, 1, p, p, p, p, None) == E_SIZE          # H bh past 2^30: the integer source coordinates
    assert pf(3, 8, 8, 2, 1, 1, None, p, p, p, None) == E_NULL
    assert pf(3, 8, 8, 2, 1, 1, p, None, p, p, None) == E_NULL
    assert pf(3, 8, 8, 2, 1, 1, p, p, None, None, None) == E_NULL
    # pixel bias backward: (C, H, W, n_cameras, bh, bw, cam, grad_out, grad_bias, stream)
    pb = L.d3ga_pixel_bias_bwd
    for bad in range(6):
        sizes = [3, 8, 8, 2, 1, 1]
        sizes[bad] = 0
        assert pb(*sizes, p, p, p, None) == E_SIZE, bad
    for bad in range(3):
        args = [p, p, p]
        args[bad] = None
        assert pb(3, 8, 8, 2, 1, 1, *args, None) == E_NULL, bad


def test_modules_match_the_reference_state_dicts(golden):
    from d3ga_amd import _lib
    from d3ga_amd.calibration import CameraCalibration, CameraPixelBias
    z = golden("calib_cases.npz")
    names = [str(s) for s in z["names"]]
    m = CameraCalibration(names)
    sd = m.state_dict()
    assert list(sd) == [str(s) for s in z["calib_state_keys"]] == ["corrections"]
    assert tuple(sd["corrections"].shape) == tuple(z["calib_state_shape"]) and sd["corrections"].dtype == torch.float32
    assert np.array_equal(sd["corrections"].numpy().astype(np.float64), z["calib_init"])
    assert m.identity_camera == str(z["calib_default_identity"]) == names[0] and m.identity_idx == 0
    assert m.n_cameras == 4 and m.cameras == names and m.cam2index == {c: i for i, c in enumerate(names)}
    assert CameraCalibration(names, "nobody").identity_camera == names[0]     # an unknown name falls back like None
    m2 = CameraCalibration(names, "cam_c")
    assert m2.identity_idx == 2
    m2.load_state_dict({"corrections": torch.randn(4, 6)}, strict=True)
    # the model's checkpoint holds it as learnable_calib.* (models/garment_net.py:44)
    holder = torch.nn.Module()
    holder.learnable_calib = CameraCalibration(names)
    holder.load_state_dict({"learnable_calib.corrections": torch.from_numpy(z["corr0"]).float()}, strict=True)
    assert m.corrections.requires_grad and m.corrections.is_leaf
    # the identity camera, by name: the input tensor itself (CPU tensors included: nothing is launched)
    x = torch.rand(7, 3)
    assert m2(x, "cam_c") is x
    img = torch.rand(3, 4, 5)
    assert m2(img, "cam_c") is img
    with pytest.raises(_lib.D3GAError):                       # GPU tensors only, no CPU fallback
        m2(x, "cam_a")
    with pytest.raises(KeyError):
        m2(x, "nobody")

    H, W = (int(v) for v in z["bias_hw"])
    pb = CameraPixelBias(H, W, int(z["bias_ds_rate"]), names)
    sd = pb.state_dict()
    assert list(sd) == [str(s) for s in z["bias_state_keys"]] == ["bias"]
    assert tuple(sd["bias"].shape) == tuple(z["bias_init_shape"]) == (4, 1, W // 8, H // 8)
    assert sd["bias"].dtype == torch.float32 and not sd["bias"].any()
    assert (pb.image_height, pb.image_width, pb.n_cameras, pb.cameras) == (H, W, 4, names)
    pb.load_state_dict({"bias": torch.from_numpy(z["bias"]).float()}, strict=True)
    assert tuple(CameraPixelBias(1022, 747, 8, names).bias.shape) == (4, 1, 93, 127)     # the Goliath size
    with pytest.raises(_lib.D3GAError):
        pb(torch.tensor([0]))


def test_python_layer_validates_on_the_host():
    from d3ga_amd import _lib
    from d3ga_amd.calibration import color_calib, pixel_bias, pixel_bias_add
    cor = torch.zeros(2, 6)
    with pytest.raises(ValueError):
        color_calib(torch.zeros(5, 4), cor, 0, 0)
    with pytest.raises(ValueError):
        color_calib(torch.zeros(2, 5, 3), cor, 0, 0, channels_first=True)
    with pytest.raises(ValueError):
        color_calib(torch.zeros(5, 3), torch.zeros(2, 5), 0, 0)
    with pytest.raises(ValueError):
        pixel_bias(torch.zeros(2, 3, 4), 0, 8, 8)
    with pytest.raises(ValueError):
        pixel_bias_add(torch.zeros(8, 8), torch.zeros(2, 1, 3, 4), 0)
    with pytest.raises(_lib.D3GAError):
        color_calib(torch.zeros(5, 3), cor, 0, 0)
    with pytest.raises(_lib.D3GAError):
        pixel_bias(torch.zeros(2, 1, 3, 4), 0, 8, 8)
