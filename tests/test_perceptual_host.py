"""CPU-side checks of the VGG perceptual loss: the float64 oracle against the reference's own output, the level plan, the
packing maps of the convolution's weight panels (a g++ build of csrc/perceptual_math.h), the weight loader, the argument
checks of the C ABI, and the qualification of every seed the GPU tests list.  Runs without a GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import perceptual_ref as pr
from conftest import ROOT

from d3ga_amd import perceptual as P


def _golden_sd(g):
    return {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w.")}


@pytest.mark.parametrize("n_layers", [5, 2])
@pytest.mark.parametrize("name", ["odd", "even"])
def test_oracle_in_float32_meets_the_reference_capture(golden, name, n_layers):
    """The restatement evaluated in float32 against the loss and dL/dpred the reference's VGGLoss returned, under the project's
    element-wise bar |a - b| <= 1e-3 |b| + 1e-6 max|b|."""
    g = golden("vgg_cases.npz")
    pred, gt = torch.from_numpy(g[f"{name}_pred"]), torch.from_numpy(g[f"{name}_gt"])
    r = pr.chain(pred, gt, _golden_sd(g), n_layers, torch.float32)
    rel, floor = pr.GOLDEN_BAR
    ref = float(g[f"{name}_loss_n{n_layers}"])
    assert abs(float(r["loss"]) - ref) <= (rel + floor) * abs(ref)
    assert pr.excess(r["grad"], g[f"{name}_grad_n{n_layers}"], rel, floor) <= 0
    assert tuple(g["widths"]) == pr.GOLDEN_WIDTHS


def test_plan_reproduces_the_reference_shapes(golden):
    g = golden("vgg_cases.npz")
    for H, W in ((512, 512), (1024, 1024), (1100, 1300), (747, 1022)):
        pl = P.plan(H, W, 5)
        assert pl.image == tuple(int(v) for v in g[f"shape_{H}x{W}"]), (H, W)
    assert P.plan(512, 512).image == (512, 512) and not P.plan(512, 512).down          # the exemption
    assert P.plan(1100, 1300).image == (550, 650)                                      # a side above 512: the crop never crops
    assert P.plan(1100, 1300).rng_draws == 2 and P.plan(1024, 1024).rng_draws == 0 and P.plan(747, 1022).rng_draws == 0
    pl = P.plan(37, 35, 5)
    assert pl.image == (18, 17) and pl.convs[-1] == (1, 1) and len(pl.convs) == 13
    assert pl.taps == ((18, 17), (9, 8), (4, 4), (2, 2), (1, 1))
    assert len(P.plan(37, 35, 2).convs) == 3 and P.plan(16, 16, 5, downsize=False).convs[-1] == (1, 1)
    with pytest.raises(ValueError):
        P.plan(16, 16, 5)                    # 8 x 8 after the downsize: nothing is left for the fourth pool
    with pytest.raises(ValueError):
        P.plan(64, 64, 6)
    # the oracle walks the same sizes
    pred, gt = pr.make_images(37, 35, 0)
    r = pr.chain(pred, gt, pr.make_weights(pr.GOLDEN_WIDTHS, 0), 5, torch.float32)
    assert tuple(tuple(t.shape[1:]) for t in r["taps"]) == pl.taps


@pytest.fixture(scope="module")
def pccheck():
    src = os.path.join(ROOT, "tests", "hostcheck", "perceptual_check.cpp")
    out_dir = os.path.join(ROOT, "tests", "hostcheck", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libperceptualcheck.so")
    deps = [src, os.path.join(ROOT, "d3ga_amd", "csrc", "perceptual_math.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", so])
    L = ctypes.CDLL(so)
    L.pc_check_panels.restype = ctypes.c_int64
    L.pc_host_panel_bytes.restype = ctypes.c_int64
    return L


@pytest.mark.parametrize("cout,cin", [(64, 3), (128, 64), (33, 5), (24, 40), (1, 1), (8, 9), (32, 16), (65, 17)])
def test_packing_maps(pccheck, cout, cin):
    """For every (co, ci, ky, kx) the input-gradient panel's slot is the forward slot of (ci, co, 2 - ky, 2 - kx), the forward
    panel's the plain one, and every K or N padding slot is zero; the library sizes the panels as the header does."""
    import d3ga_amd
    assert pccheck.pc_check_panels(cout, cin) == 0
    L = d3ga_amd.lib()
    assert L.d3ga_vgg_panel_bytes(cin, cout) == pccheck.pc_host_panel_bytes(cin, cout)
    assert L.d3ga_vgg_panel_bytes(cout, cin) == pccheck.pc_host_panel_bytes(cout, cin)
    assert pccheck.pc_host_panel_bytes(cin, cout) == 3 * 16 * 2 * pccheck.pc_host_ksteps(cin) * 32 * ((cout + 31) // 32)


def test_weight_loader_accepts_both_key_styles_and_rejects_bad_dicts(tmp_path):
    a, b = pr.make_weights(pr.NARROW_WIDTHS, 1, "features"), pr.make_weights(pr.NARROW_WIDTHS, 1, "plain")
    assert "features.0.weight" in a and "0.weight" in b
    la, lb = P.load_vgg_weights(a, 5), P.load_vgg_weights(b, 5)
    assert len(la) == 13 and all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(la, lb))
    assert len(P.load_vgg_weights(a, 2)) == 3
    path = tmp_path / "vgg.pt"
    torch.save(a, path)
    assert torch.equal(P.load_vgg_weights(str(path), 1)[0][0], a["features.0.weight"])
    mod = P.VGGLoss(2, a)
    assert mod.widths == pr.NARROW_WIDTHS[:3] and not list(mod.parameters()) and not mod.state_dict()
    assert len(list(mod.buffers())) == 2 * 3 + 1
    missing = dict(a)
    del missing["features.5.bias"]
    with pytest.raises(KeyError):
        P.load_vgg_weights(missing, 5)
    assert len(P.load_vgg_weights(missing, 1)) == 1          # what n_layers does not need is not asked for
    for key, shape in (("features.2.weight", (8, 9, 3, 3)), ("features.2.weight", (8, 8, 3)), ("features.2.weight", (8, 8, 5, 5)),
                       ("features.2.bias", (9,)), ("features.0.weight", (8, 4, 3, 3))):
        bad = dict(a)
        bad[key] = torch.zeros(shape)
        with pytest.raises(ValueError):
            P.load_vgg_weights(bad, 5)
    bad = dict(a)
    bad["features.0.bias"] = torch.zeros(8, dtype=torch.int64)
    with pytest.raises(ValueError):
        P.load_vgg_weights(bad, 5)
    with pytest.raises(TypeError):
        P.load_vgg_weights(3, 5)
    with pytest.raises(ValueError):
        P.VGGLoss(0, a)


def test_default_weights_need_torchvision_and_say_so(monkeypatch):
    import sys
    monkeypatch.setitem(sys.modules, "torchvision", None)      # `import torchvision` raises ImportError
    with pytest.raises(ImportError, match="weights="):
        P.VGGLoss()


def test_ops_refuse_cpu_tensors():
    from d3ga_amd._lib import D3GAError
    sd = pr.make_weights(pr.NARROW_WIDTHS, 0)
    with pytest.raises(D3GAError):
        P.VGGLoss(1, sd)(torch.zeros(3, 8, 8), torch.zeros(3, 8, 8))
    with pytest.raises(D3GAError):
        P.maxpool2(torch.zeros(4, 4, 2))


def test_entry_points_refuse_bad_arguments_no_gpu_needed():
    """Every refusal below returns before any launch: the calls run on a machine without a GPU."""
    import d3ga_amd
    L = d3ga_amd.lib()
    E_NULL, E_SIZE, E_CONFIG = -1, -2, -3
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)
    assert L.d3ga_vgg_panel_bytes(0, 8) == E_SIZE and L.d3ga_vgg_panel_bytes(8, -1) == E_SIZE
    assert L.d3ga_vgg_pack_weights(0, 3, p, 0, p, None) == E_SIZE
    assert L.d3ga_vgg_pack_weights(8, 3, None, 0, p, None) == E_NULL
    assert L.d3ga_vgg_pack_weights(8, 3, p, 0, None, None) == E_NULL
    assert L.d3ga_vgg_pack_weights(8, 3, p, 2, p, None) == E_CONFIG
    assert L.d3ga_vgg_pack_weights(8, 3, p, 0, odd, None) == E_CONFIG
    conv = L.d3ga_vgg_conv3x3
    assert conv(0, 4, 3, 8, p, None, p, None, 1, 0, p, None) == E_SIZE
    assert conv(4, 4, 0, 8, p, None, p, None, 1, 0, p, None) == E_SIZE
    assert conv(4, 4, 3, -2, p, None, p, None, 1, 0, p, None) == E_SIZE
    assert conv(65536, 65536, 3, 8, p, None, p, None, 1, 0, p, None) == E_SIZE        # H W past INT32_MAX
    assert conv(4096, 4096, 3, 512, p, None, p, None, 1, 0, p, None) == E_SIZE         # H W Cout past INT32_MAX
    assert conv(4, 4, 3, 8, None, None, p, None, 1, 0, p, None) == E_NULL
    assert conv(4, 4, 3, 8, p, None, None, None, 1, 0, p, None) == E_NULL
    assert conv(4, 4, 3, 8, p, None, p, None, 1, 0, None, None) == E_NULL
    q = ctypes.cast((ctypes.c_float * 64)(), ctypes.c_void_p)
    assert conv(4, 4, 3, 8, p, None, q, None, 2, 0, q, None) == E_CONFIG
    assert conv(4, 4, 3, 8, p, None, q, None, 1, 3, q, None) == E_CONFIG
    assert conv(4, 4, 3, 8, odd, None, q, None, 1, 0, q, None) == E_CONFIG
    assert conv(4, 4, 3, 8, p, odd, q, None, 0, 0, q, None) == E_CONFIG
    assert conv(4, 4, 3, 8, p, None, p, None, 1, 0, p, None) == E_CONFIG              # y aliases x
    assert conv(4, 4, 3, 8, p, q, p, None, 0, 0, q, None) == E_CONFIG                 # y aliases the mask
    for fn in (L.d3ga_vgg_maxpool2_fwd,):
        assert fn(1, 4, 2, p, q, None) == E_SIZE and fn(4, 4, 0, p, q, None) == E_SIZE
        assert fn(4, 4, 2, None, q, None) == E_NULL and fn(4, 4, 2, p, None, None) == E_NULL
    assert L.d3ga_vgg_maxpool2_bwd(4, 1, 2, p, q, q, None) == E_SIZE
    assert L.d3ga_vgg_maxpool2_bwd(4, 4, 2, p, None, q, None) == E_NULL
    for fn in (L.d3ga_vgg_box_down2_fwd, L.d3ga_vgg_box_down2_bwd):
        assert fn(3, 1, 8, 1, p, q, None) == E_SIZE and fn(0, 8, 8, 1, p, q, None) == E_SIZE
        assert fn(3, 8, 8, 1, None, q, None) == E_NULL and fn(3, 8, 8, 1, p, None, None) == E_NULL
        assert fn(3, 8, 8, 2, p, q, None) == E_CONFIG
    out = (ctypes.c_int64 * 3)()
    sb = L.d3ga_vgg_scratch_bytes
    assert sb(64, 64, 1, 5, None, None) == E_NULL
    assert sb(0, 64, 1, 5, None, out) == E_SIZE and sb(16, 16, 1, 5, None, out) == E_SIZE      # too small for the pools
    assert sb(64, 64, 1, 0, None, out) == E_CONFIG and sb(64, 64, 1, 6, None, out) == E_CONFIG and sb(64, 64, 2, 5, None, out) == E_CONFIG
    bad = (ctypes.c_int32 * 13)(*([8] * 12 + [0]))
    assert sb(64, 64, 1, 5, bad, out) == E_SIZE and sb(64, 64, 1, 4, bad, out) == 0
    # sizes: VGG19 at 32 x 32 -> 16 x 16: the saved section holds the image, 13 activations, 4 pooled maps and 5 tap gradients
    assert sb(32, 32, 1, 5, None, out) == 0
    a256 = lambda n: (n + 255) & ~255
    pl = P.plan(32, 32, 5)
    want = a256(4 * 3 * 16 * 16)
    for i, ((h, w), c) in enumerate(zip(pl.convs, pr.VGG19_WIDTHS)):
        if i in pr.POOL_BEFORE:
            want += a256(4 * h * w * pr.VGG19_WIDTHS[i - 1])
        want += a256(4 * h * w * c) * (2 if i in pr.TAPS else 1)
    big = 16 * 16 * 64
    assert (out[0], out[1], out[2]) == (want, 2 * a256(4 * big) + a256(4 * 2048) + 256, 2 * a256(4 * big))
    assert P.scratch_bytes(32, 32, True, 5, pr.VGG19_WIDTHS) == (out[0], out[1], out[2])


def _seed_cases():
    cases = [(hw, s, s) for hw, seeds in pr.NARROW_SEEDS.items() for s in seeds]
    hw, ws, imgs = pr.NARROW_BATCH
    return cases + [(hw, ws, i) for i in imgs]


@pytest.mark.parametrize("hw,wseed,iseed", _seed_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_every_listed_seed_qualifies(hw, wseed, iseed):
    """No decision of the gradient (ReLU sign, pool winner, sign of source - target) can flip inside the device's allowance:
    every margin is >= 16 x the float32 evaluation's own error, 4 x what the device is allowed."""
    ok, worst = pr.qualify(*pr.make_images(hw[0], hw[1], iseed), pr.make_weights(pr.NARROW_WIDTHS, wseed), 5)
    assert ok, worst


def test_seed_lists_are_long_enough_and_the_golden_case_qualifies(golden):
    assert all(len(set(s)) >= 4 for s in pr.NARROW_SEEDS.values()) and set(pr.NARROW_SEEDS) == {(37, 53), (40, 56)}
    g = golden("vgg_cases.npz")
    for name in ("odd", "even"):
        ok, worst = pr.qualify(torch.from_numpy(g[f"{name}_pred"]), torch.from_numpy(g[f"{name}_gt"]), _golden_sd(g), 5)
        assert ok, (name, worst)
