"""The LPIPS (VGG) metric without a GPU: the oracle's own known answers (tests/lpips_ref.py -- the formula pinned from first
principles, since parity with the `lpips` package is unpinned), the size plan, the weight loader in both key layouts and its
refusals, the refusals of every new C entry point before any launch, the compat import statement, and the stand-alone g++
build of csrc/lpips_math.h (tests/hostcheck/lpips_check.cpp)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

import lpips_ref as lr
import perceptual_ref as pr
from conftest import ROOT

E_NULL, E_SIZE, E_CONFIG = -1, -2, -3            # D3GA_E_* (include/d3ga.h)


def _L():
    from d3ga_amd import lpips
    return lpips


# ---- the oracle itself ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_oracle_distance_known_answers(dtype):
    C = 7
    lin = torch.tensor([0.3, 0.11, -0.05, 0.07, 0.2, 0.13, 0.017], dtype=dtype)
    eye = torch.eye(C, dtype=dtype)
    d = lambda a, b: lr.tap_distance(a.view(1, C, 1, 1), b.view(1, C, 1, 1), lin).item()
    for i in range(C):
        for j in range(C):
            want = 0.0 if i == j else (lin[i] + lin[j]).item()
            assert d(eye[i], eye[j]) == pytest.approx(want, rel=1e-6 if dtype == torch.float32 else 1e-9, abs=0)     # one-hot pair
        assert d(torch.zeros(C, dtype=dtype), eye[i]) == pytest.approx(lin[i].item(), rel=1e-6)                     # a zero side: lin_j, no NaN
    g = torch.Generator().manual_seed(0)
    a, b = torch.rand(C, generator=g).to(dtype) + 0.1, torch.rand(C, generator=g).to(dtype) + 0.1
    assert d(a, a) == 0.0 and d(torch.zeros(C, dtype=dtype), torch.zeros(C, dtype=dtype)) == 0.0                    # exactly
    assert d(3.7 * a, 0.31 * b) == pytest.approx(d(a, b), rel=1e-5 if dtype == torch.float32 else 1e-9)             # scale invariance
    if dtype == torch.float32:          # powers of two: exact where 1e-10 is below half an ulp of the norms (float64 sees it: 1e-10 relative)
        assert d(4 * a, 0.5 * b) == d(a, b)


@pytest.mark.parametrize("normalize", [False, True])
def test_oracle_chain_properties(normalize):
    sd = lr.make_weights(pr.NARROW_WIDTHS, 0)
    fake, target = pr.make_images(16, 19, 0, n=2)
    r = lr.chain(fake, target, sd, normalize)
    assert [tuple(m.shape) for m in r["maps"]] == [(2, 16, 19), (2, 8, 9), (2, 4, 4), (2, 2, 2), (2, 1, 1)]
    assert [t.shape[1] for t in r["taps_a"]] == [8, 20, 40, 33, 48]
    assert r["value"].shape == (2,) and bool((r["value"] != 0).all()) and bool(torch.isfinite(r["value"]).all())
    same = lr.chain(fake, fake, sd, normalize)
    assert all(not m.any() for m in same["maps"]) and not same["value"].any()          # d(x, x) == 0, exactly
    # the scaling layer: normalize feeds 2 x - 1; without it the [0, 1] image goes in as it is (the reference's quirk)
    x = torch.rand(3, 4, 5, dtype=torch.float64)
    for c in range(3):
        assert torch.allclose(lr.scale_input(x, False)[c], (x[c] - lr.SHIFT[c]) / lr.SCALE[c], rtol=0, atol=1e-15)
        assert torch.allclose(lr.scale_input(x, True)[c], (2 * x[c] - 1 - lr.SHIFT[c]) / lr.SCALE[c], rtol=0, atol=1e-15)
    other = lr.chain(fake, target, sd, not normalize)
    assert not torch.equal(other["value"], r["value"])
    # the float32 evaluation stays near the float64 one
    r32 = lr.chain(fake, target, sd, normalize, torch.float32)
    assert lr.e32_rel(r32["value"], r["value"]) < 1e-4


def test_every_listed_seed_qualifies():
    assert tuple(lr.NARROW_SEEDS) == lr.NARROW_SIZES
    for hw, by_setting in lr.NARROW_SEEDS.items():
        for normalize in (False, True):
            assert len(by_setting[normalize]) >= 2
            for s in by_setting[normalize]:
                ok, floor, spread = lr.qualify(pr.NARROW_WIDTHS, *hw, s, normalize)
                print(hw, s, normalize, f"smallest e32 {floor:.1f} x 2^-24, reordered / e32 <= {spread:.2f}")
                assert ok, (hw, s, normalize, floor, spread)
    (H, W), s = lr.VGG16_CASE
    assert lr.qualify(lr.VGG16_WIDTHS, H, W, s, False)[0]
    # and the criterion does refuse: the single pixel of this last map is a lucky draw (e32 0.4 x 2^-24)
    assert not lr.qualify(pr.NARROW_WIDTHS, 16, 16, 4, False)[0]


# ---- the size plan ----------------------------------------------------------------------------------------------------------

def test_size_plan():
    L = _L()
    assert L.plan(16, 16).taps == ((16, 16), (8, 8), (4, 4), (2, 2), (1, 1))
    assert L.plan(37, 53).taps == ((37, 53), (18, 26), (9, 13), (4, 6), (2, 3))        # odd at every level
    assert len(L.plan(37, 53).convs) == 13 and L.plan(37, 53).convs[7] == (4, 6)
    for hw in ((15, 40), (40, 15), (0, 16), (16, -1)):
        with pytest.raises(ValueError, match="too small"):
            L.plan(*hw)
    assert L.CONV_KEYS == lr.CONV_KEYS and L.TAPS == lr.TAPS and L.POOL_BEFORE == lr.POOL_BEFORE and L.VGG16_WIDTHS == lr.VGG16_WIDTHS
    assert L.SHIFT == lr.SHIFT and L.SCALE == lr.SCALE


def test_scratch_bytes_follow_the_plan():
    from d3ga_amd import _lib
    L = _L()
    lib = _lib.lib()
    out = (ctypes.c_int64 * 3)()
    a256 = lambda n: (n + 255) & ~255
    for B, H, W, widths in ((1, 16, 16, lr.VGG16_WIDTHS), (2, 37, 53, pr.NARROW_WIDTHS), (1, 747, 1022, lr.VGG16_WIDTHS)):
        pl = L.plan(H, W)
        big = max([2 * B * H * W * 3] + [2 * B * h * w * c for (h, w), c in zip(pl.convs, widths)])
        want = (2 * a256(4 * big) + a256(4 * B * _lib.LPIPS_PARTIALS), a256(4 * big), a256(4 * B * _lib.LPIPS_PARTIALS))
        assert L.scratch_bytes(B, H, W, widths) == want
        if widths is lr.VGG16_WIDTHS:                                          # NULL widths: VGG16's
            assert lib.d3ga_lpips_scratch_bytes(B, H, W, None, out) == 0 and tuple(out) == want
    assert L.scratch_bytes(1, 747, 1022, lr.VGG16_WIDTHS)[1] == a256(4 * 2 * 747 * 1022 * 64)
    arr = (ctypes.c_int32 * 13)(*lr.VGG16_WIDTHS)
    assert lib.d3ga_lpips_scratch_bytes(1, 64, 64, arr, None) == E_NULL
    for B, H, W in ((0, 64, 64), (-1, 64, 64), (65536, 64, 64), (1, 15, 40), (1, 40, 15), (1, 0, 64), (1, 32768, 32768), (64, 4096, 4096)):
        assert lib.d3ga_lpips_scratch_bytes(B, H, W, arr, out) == E_SIZE, (B, H, W)
    bad = (ctypes.c_int32 * 13)(*([8] * 12 + [0]))
    assert lib.d3ga_lpips_scratch_bytes(1, 64, 64, bad, out) == E_SIZE
    wide = (ctypes.c_int32 * 13)(*([8] * 12 + [513]))                          # a tap wider than the distance kernel holds
    assert lib.d3ga_lpips_scratch_bytes(1, 64, 64, wide, out) == E_SIZE
    wide_inner = (ctypes.c_int32 * 13)(*([8] * 2 + [600] + [8] * 10))          # not a tap: any width
    assert lib.d3ga_lpips_scratch_bytes(1, 64, 64, wide_inner, out) == 0
    with pytest.raises(ValueError):
        L.scratch_bytes(1, 15, 40, lr.VGG16_WIDTHS)
    assert _lib.LPIPS_PARTIALS == int(re.search(r"#define\s+D3GA_LPIPS_PARTIALS\s+(\d+)", open(os.path.join(ROOT, "include", "d3ga.h")).read()).group(1))


# ---- weights -----------------------------------------------------------------------------------------------------------------

def test_both_weight_layouts_load_to_identical_tensors(tmp_path):
    L = _L()
    tv = lr.make_weights(pr.NARROW_WIDTHS, 1, "torchvision", "lin")
    pk = lr.make_weights(pr.NARROW_WIDTHS, 1, "package", "lin")
    pk2 = lr.make_weights(pr.NARROW_WIDTHS, 1, "package", "lins")
    assert "features.17.weight" in tv and "net.slice4.17.weight" in pk and "net.slice1.2.bias" in pk and "net.slice5.28.bias" in pk
    assert "lin4.model.1.weight" in pk and "lins.4.model.1.weight" in pk2 and "features.16.weight" not in tv
    pa, la = L.load_lpips_weights(tv)
    assert len(pa) == 13 and len(la) == 5 and tuple(int(w.shape[0]) for w, _ in pa) == pr.NARROW_WIDTHS
    assert [l.shape[0] for l in la] == [8, 20, 40, 33, 48] and all(l.dim() == 1 and bool((l < 0).any()) for l in la)
    for other in (pk, pk2):
        pb, lb = L.load_lpips_weights(other)
        assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(pa, pb))
        assert all(torch.equal(x, y) for x, y in zip(la, lb))
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(pa, lr.pairs_of(tv)))
    path = tmp_path / "lpips.pt"
    torch.save(pk, path)
    pc, lc = L.load_lpips_weights(str(path))
    assert torch.equal(pc[12][0], pa[12][0]) and torch.equal(lc[3], la[3])
    mod = L.LPIPS("vgg", tv)
    assert mod.widths == pr.NARROW_WIDTHS and mod.normalize is False and not list(mod.parameters()) and not mod.state_dict()
    assert len(list(mod.buffers())) == 2 * 13 + 5
    assert L.LPIPS(weights=path, normalize=True).normalize is True
    # float64 weights are taken as float32
    assert L.load_lpips_weights({k: v.double() for k, v in tv.items()})[0][0][0].dtype == torch.float32


def test_malformed_weights_raise_with_the_key_named():
    L = _L()
    tv = lr.make_weights(pr.NARROW_WIDTHS, 2)
    for key in ("features.17.bias", "features.0.weight", "lin3.model.1.weight"):
        bad = dict(tv)
        del bad[key]
        with pytest.raises(KeyError, match=re.escape(key)):
            L.load_lpips_weights(bad)
    pk = lr.make_weights(pr.NARROW_WIDTHS, 2, "package", "lins")
    del pk["net.slice3.14.weight"]
    with pytest.raises(KeyError, match=re.escape("net.slice3.14.weight")):
        L.load_lpips_weights(pk)
    for key, t in (("features.2.weight", torch.zeros(8, 9, 3, 3)), ("features.2.weight", torch.zeros(8, 8, 3)),
                   ("features.2.weight", torch.zeros(8, 8, 5, 5)), ("features.2.bias", torch.zeros(9)), ("features.0.weight", torch.zeros(8, 4, 3, 3)),
                   ("lin1.model.1.weight", torch.zeros(1, 21, 1, 1)), ("lin1.model.1.weight", torch.zeros(20)),
                   ("lin0.model.1.weight", torch.zeros(1, 8, 1, 1, dtype=torch.int64)), ("features.28.bias", torch.zeros(48, dtype=torch.int32))):
        bad = dict(tv)
        bad[key] = t
        with pytest.raises(ValueError, match=re.escape(key)):
            L.load_lpips_weights(bad)
    wide = lr.make_weights((8,) * 12 + (520,), 0)
    with pytest.raises(ValueError, match=re.escape("lin4.model.1.weight")):
        L.load_lpips_weights(wide)
    with pytest.raises(TypeError):
        L.load_lpips_weights(3)
    for net in ("alex", "squeeze", "vgg19"):
        with pytest.raises(NotImplementedError, match=net):
            L.LPIPS(net, tv)


def test_default_weights_come_from_the_environment_variable_only(monkeypatch, tmp_path):
    L = _L()
    monkeypatch.delenv("D3GA_LPIPS_WEIGHTS", raising=False)
    with pytest.raises(ImportError, match="D3GA_LPIPS_WEIGHTS") as e:
        L.LPIPS()
    assert "features.K" in str(e.value) and "net.slice" in str(e.value) and "weights=" in str(e.value)
    path = tmp_path / "w.pt"
    torch.save(lr.make_weights(pr.NARROW_WIDTHS, 3, "package"), path)
    monkeypatch.setenv("D3GA_LPIPS_WEIGHTS", str(path))
    assert L.LPIPS("vgg").widths == pr.NARROW_WIDTHS


def test_vgg_loader_is_the_same_function_over_another_key_tuple():
    """load_vgg_weights (VGG19 keys) and the LPIPS loader (VGG16 keys) share perceptual.load_conv_chain."""
    from d3ga_amd import perceptual as P
    sd19 = pr.make_weights(pr.NARROW_WIDTHS, 1)
    a = P.load_vgg_weights(sd19, 5)
    b = P.load_conv_chain(sd19, P.CONV_KEYS)
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a, b))
    with pytest.raises(KeyError, match="features.17.weight"):
        P.load_conv_chain(sd19, _L().CONV_KEYS)                    # a VGG19 dict has no features.17


# ---- the Python layer's refusals ------------------------------------------------------------------------------------------

def test_python_layer_validates_on_the_host():
    from d3ga_amd._lib import D3GAError
    L = _L()
    mod = L.LPIPS("vgg", lr.make_weights(pr.NARROW_WIDTHS, 0))
    with pytest.raises(ValueError, match="too small"):
        mod(torch.zeros(3, 15, 40), torch.zeros(3, 15, 40))
    with pytest.raises(ValueError):
        mod(torch.zeros(3, 16, 16), torch.zeros(3, 16, 17))
    with pytest.raises(ValueError):
        mod(torch.zeros(1, 16, 16), torch.zeros(1, 16, 16))
    with pytest.raises(ValueError):
        mod(torch.zeros(3, 16, 16, dtype=torch.float64), torch.zeros(3, 16, 16, dtype=torch.float64))
    with pytest.raises(D3GAError):                                  # no CPU fall-back
        mod(torch.zeros(3, 16, 16), torch.zeros(3, 16, 16))
    with pytest.raises(D3GAError):
        L.tap_distance(torch.zeros(1, 2, 2, 4), torch.zeros(1, 2, 2, 4), torch.zeros(4))
    with pytest.raises(D3GAError):
        L.scale_input(torch.zeros(1, 3, 2, 2))


# ---- the C entry points ---------------------------------------------------------------------------------------------------

def test_entry_points_refuse_bad_arguments_before_any_launch():
    """The refusals happen before any HIP call: host buffers stand in for device memory and are never touched."""
    from d3ga_amd import _lib
    L = _lib.lib()
    bufs = [(ctypes.c_float * 4096)() for _ in range(7)]
    a, b, lin, mp, part, val, pan = (ctypes.c_void_p((ctypes.addressof(x) + 15) & ~15) for x in bufs)
    odd = lambda p: ctypes.c_void_p(p.value + 2)
    inside = lambda p: ctypes.c_void_p(p.value + 4)

    # d3ga_lpips_input
    ok = dict(N=1, H=2, W=2, normalize=0, img=a, out=b)
    call = lambda **kw: L.d3ga_lpips_input(*{**ok, **kw}.values(), None)
    for name in ("N", "H", "W"):
        assert call(**{name: 0}) == E_SIZE and call(**{name: -2}) == E_SIZE, name
    assert call(H=2 ** 16, W=2 ** 16) == E_SIZE and call(N=2 ** 12, H=2 ** 10, W=2 ** 10) == E_SIZE       # N H W 3 past INT32_MAX
    assert call(img=None) == E_NULL and call(out=None) == E_NULL
    assert call(normalize=2) == E_CONFIG and call(normalize=-1) == E_CONFIG
    assert call(img=odd(a)) == E_CONFIG and call(out=odd(b)) == E_CONFIG
    assert call(out=a) == E_CONFIG and call(out=inside(a)) == E_CONFIG                                   # in place

    # d3ga_lpips_tap
    ok = dict(B=1, h=2, w=2, C=8, a=a, b=b, lin=lin, map=mp, partials=part, value=val, accumulate=0)
    call = lambda **kw: L.d3ga_lpips_tap(*{**ok, **kw}.values(), None)
    for name in ("B", "h", "w", "C"):
        assert call(**{name: 0}) == E_SIZE and call(**{name: -1}) == E_SIZE, name
    assert call(C=513) == E_SIZE and call(B=65536) == E_SIZE and call(h=2 ** 16, w=2 ** 16) == E_SIZE
    assert call(B=16, h=2 ** 12, w=2 ** 12, C=8) == E_SIZE                                               # B h w C past INT32_MAX
    for name in ("a", "b", "lin", "partials", "value"):
        assert call(**{name: None}) == E_NULL, name
    assert call(accumulate=2) == E_CONFIG and call(accumulate=-1) == E_CONFIG
    for name, p in (("a", a), ("b", b), ("lin", lin), ("map", mp), ("partials", part), ("value", val)):
        assert call(**{name: odd(p)}) == E_CONFIG, name
    for out_name in ("map", "partials", "value"):                     # an output inside an input or another output
        for src in (a, b, lin):
            assert call(**{out_name: src}) == E_CONFIG and call(**{out_name: inside(src)}) == E_CONFIG, out_name
    assert call(map=part) == E_CONFIG and call(value=inside(part)) == E_CONFIG and call(map=val) == E_CONFIG

    # the batched convolution and pool: the single-image refusals, and N
    conv = L.d3ga_vgg_conv3x3_n
    okc = dict(N=2, H=4, W=4, cin=3, cout=8, x=a, mask_y=None, panel=pan, bias=None, relu=1, accumulate=0, y=b)
    call = lambda **kw: conv(*{**okc, **kw}.values(), None)
    for name in ("N", "H", "W", "cin", "cout"):
        assert call(**{name: 0}) == E_SIZE and call(**{name: -2}) == E_SIZE, name
    assert call(N=2 ** 16, H=2 ** 8, W=2 ** 8) == E_SIZE                                                 # N H W cout past INT32_MAX
    assert call(N=1, H=65536, W=65536) == E_SIZE and call(N=16, H=4096, W=4096, cout=8) == E_SIZE
    assert call(N=8, H=4096, W=4096, cin=3, cout=16) == E_SIZE                                           # 2^31 elements exactly
    for name in ("x", "panel", "y"):
        assert call(**{name: None}) == E_NULL, name
    assert call(relu=2) == E_CONFIG and call(accumulate=3) == E_CONFIG
    assert call(x=inside(a)) == E_CONFIG and call(mask_y=inside(a), relu=0) == E_CONFIG and call(panel=inside(pan)) == E_CONFIG
    assert call(y=a) == E_CONFIG and call(mask_y=b, relu=0) == E_CONFIG                                  # y aliases x / the mask
    pool = L.d3ga_vgg_maxpool2_fwd_n
    assert pool(0, 4, 4, 2, a, b, None) == E_SIZE and pool(2, 1, 4, 2, a, b, None) == E_SIZE and pool(2, 4, 4, 0, a, b, None) == E_SIZE
    assert pool(2 ** 10, 2 ** 11, 2 ** 11, 1, a, b, None) == E_SIZE
    assert pool(2, 4, 4, 2, None, b, None) == E_NULL and pool(2, 4, 4, 2, a, None, None) == E_NULL
    assert pool(2, 4, 4, 2, a, a, None) == E_CONFIG
    assert not any(any(x) for x in bufs)


def test_new_abi_surface():
    from d3ga_amd import _lib
    src = open(os.path.join(ROOT, "include", "d3ga.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], capture_output=True, text=True, check=True).stdout
    for name, nargs in (("d3ga_vgg_conv3x3_n", 13), ("d3ga_vgg_maxpool2_fwd_n", 7), ("d3ga_lpips_input", 7), ("d3ga_lpips_tap", 12),
                        ("d3ga_lpips_scratch_bytes", 5)):
        assert name in _lib.EXPORTS and len(_lib._SIGNATURES[name][0]) == nargs, name
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert hasattr(_lib.lib(), name)
        assert re.search(r"\bT %s$" % name, out, flags=re.M), name
    assert _lib.ABI_VERSION == 112 and re.search(r"#define\s+D3GA_VERSION\s+112\b", src) and _lib.lib().d3ga_version() == 112
    build = open(os.path.join(ROOT, "d3ga_amd", "csrc", "build.py")).read()
    assert '"lpips.hip"' in build and '"lpips_math.h"' in build
    import d3ga_amd
    assert d3ga_amd.LPIPS is _L().LPIPS and "LPIPS" in d3ga_amd.__all__


def test_compat_import_statement():
    """recorder/heatmap.py:9, 13: `import lpips` ... `lpips.LPIPS("vgg")` resolves against compat/."""
    compat = os.path.join(ROOT, "compat")
    saved = sys.modules.pop("lpips", None)
    sys.path.insert(0, compat)
    try:
        import lpips
        assert lpips.LPIPS is _L().LPIPS and os.path.dirname(lpips.__file__) == os.path.join(compat, "lpips")
        with pytest.raises(NotImplementedError):
            lpips.LPIPS("alex", {})
    finally:
        sys.path.remove(compat)
        sys.modules.pop("lpips", None)
        if saved is not None:
            sys.modules["lpips"] = saved


# ---- csrc/lpips_math.h on the CPU -----------------------------------------------------------------------------------------

def test_lpips_math_hostcheck_program():
    src = os.path.join(ROOT, "tests", "hostcheck", "lpips_check.cpp")
    out_dir = os.path.join(ROOT, "tests", "hostcheck", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "lpips_check")
    deps = [src, os.path.join(ROOT, "d3ga_amd", "csrc", "lpips_math.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:]
