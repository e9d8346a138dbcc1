"""The evaluation tail without a GPU: the float64 numpy oracle (tests/eval_ref.py) against the reference's own psnr, ssim-free
compute_heatmap / compute_errors and dist_to_rgb (tests/golden/eval_cases.npz, tools/gen_eval_golden.py); the library's jet
table against the reference's; the CPU build of csrc/eval_math.h -- the text the kernel runs -- against the oracle under the
bars of the GPU tests; the mean of per-channel PSNRs against the pooled one; the ABI surface and its refusals; the Python
layer's ValueErrors and the line Evaluator.write writes."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import eval_ref as er
from conftest import ROOT, ptr

E_NULL, E_SIZE, E_CONFIG = -1, -2, -3            # D3GA_E_* (include/d3ga.h)
BG_WHITE, COMPOSED, ALPHA3, BOUNDARY_F32 = 1, 2, 4, 8
COMPOSE_BAR = 1e-6      # the bar compose_target takes (test_gpu_image_tail.py): three float32 roundings on values <= 2
# |psnr - psnr64| <= 1e-3 dB: d dB = (10 / ln 10) delta with delta <= (n + 3) 2^-24 for the longest chain of n additions a term
# passes through; n <= 154 in eval.hip (42 up to a 4K frame), and the bar's derivation allows up to 2048 (5.3e-4 dB)
PSNR_BAR = 1e-3
PAIRS = ("a", "b", "c", "wide")


@pytest.fixture(scope="module")
def evalcheck():
    src = os.path.join(ROOT, "tests", "hostcheck", "eval_host.cpp")
    out_dir = os.path.join(ROOT, "tests", "hostcheck", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libeval_host.so")
    deps = [src, os.path.join(ROOT, "d3ga_amd", "csrc", "eval_math.h"), os.path.join(ROOT, "include", "d3ga.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", so])
    return ctypes.CDLL(so)


def _host(lib, pred, image, alpha=None, boundary=None, flags=0, outputs=("target", "gt", "heat", "partials")):
    """hc_eval_frames + hc_eval_finish (the kernels' loops on the CPU) -> dict of arrays."""
    B, _, H, W = pred.shape
    pred, image = np.ascontiguousarray(pred, np.float32), np.ascontiguousarray(image, np.float32)
    if alpha is None:
        flags |= COMPOSED
        outputs = [o for o in outputs if o in ("heat", "partials")]
    else:
        alpha = np.ascontiguousarray(alpha, np.float32)
        flags |= (ALPHA3 if alpha.shape[1] == 3 else 0) | (BOUNDARY_F32 if boundary.dtype == np.float32 else 0)
        boundary = np.ascontiguousarray(boundary)
        assert boundary.dtype in (np.uint8, np.bool_, np.float32)
    npart = lib.hc_eval_partials(H, W)
    out = {"target": np.full((B, 3, H, W), np.nan, np.float32), "gt": np.full((B, 4, H, W), np.nan, np.float32),
           "heat": np.full((B, 3, H, W), np.nan, np.float32), "partials": np.full((B, 3, npart), np.nan, np.float32)}
    out = {k: v for k, v in out.items() if k in outputs}
    assert lib.hc_eval_frames(B, H, W, flags, ptr(pred), ptr(image), ptr(alpha), ptr(boundary), ptr(out.get("target")), ptr(out.get("gt")),
                              ptr(out.get("heat")), ptr(out.get("partials"))) == 0
    if "partials" in out:
        out["psnr"], out["psnr_channels"] = np.empty(B, np.float32), np.empty((B, 3), np.float32)
        lib.hc_eval_finish(B, H, W, ptr(out["partials"]), ptr(out["psnr"]), ptr(out["psnr_channels"]))
    return out


def test_oracle_equals_the_reference(golden):
    z = golden("eval_cases.npz")
    table = er.jet_table_ref()
    assert np.array_equal(table[:256], z["table"]) and z["table"].shape == (256, 3) and z["table"].dtype == np.uint8
    assert float(z["wide_gt"].min()) >= 0 and (float(z["wide_pred"].max()) > 1 and float(z["wide_pred"].min()) < 0)
    for name in PAIRS:
        gt, pred = z[f"{name}_gt"], z[f"{name}_pred"]
        assert gt.dtype == np.float32 and gt.shape[0] == 3
        got = float(er.psnr_ref(gt, pred))
        print(f"{name}: psnr oracle {got:.6f} reference {float(z[f'{name}_psnr']):.6f}")
        assert abs(got - float(z[f"{name}_psnr"])) <= PSNR_BAR
        assert float(np.abs(er.psnr_channels_ref(gt, pred) - z[f"{name}_psnr_channels"][:, 0]).max()) <= PSNR_BAR
        # the reference's heat map (from its float32 errors) under the edge rule, both layouts
        n_open, n = er.check_heat(z[f"{name}_heat"], gt, pred, table)
        er.check_heat(np.moveaxis(z[f"{name}_heat_hwc"], -1, 0), gt, pred, table)
        print(f"{name}: {n_open} of {n} pixels within {er.EDGE} of a bin edge")
    assert (er.errors_ref(z["wide_gt"], z["wide_pred"]) > 1).any()
    # the ramp and the edge values: entry for entry
    ramp = z["ramp"]
    assert ramp.shape == (4001,) and ramp.dtype == np.float32 and ramp[0] == 0 and abs(float(ramp[-1]) - 1.8) < 1e-6
    assert np.array_equal(table[er.heat_bins(ramp)], z["ramp_heat"])
    edge = z["edge"]
    assert edge[0] == 0 and edge[1] == 1 and edge[2] < 1 < edge[3] and np.isnan(edge[4])
    assert np.array_equal(er.heat_bins(edge)[:5], [0, 255, 255, 255, er.BAD])
    assert np.array_equal(table[er.heat_bins(edge)], z["edge_heat"])
    assert np.array_equal(z["edge_heat"][4], [0, 0, 0])       # matplotlib's "bad" colour, times 255


def test_library_jet_table_equals_the_reference(golden, evalcheck):
    from d3ga_amd.evaluation import jet_table
    want = golden("eval_cases.npz")["table"]
    got = jet_table().numpy()                                 # d3ga_eval_jet_table: the table the kernel's LDS copy is built from
    assert got.shape == (257, 3) and got.dtype == np.uint8
    assert np.array_equal(got[:256], want) and np.array_equal(got[256], [0, 0, 0])
    host = np.empty((257, 3), np.uint8)
    evalcheck.hc_eval_jet_table(ptr(host))                    # the same header through g++
    assert np.array_equal(host, got)
    assert np.array_equal(er.jet_table_ref(), got)
    # uint8 / 255 in float32 (heatmap.py:47) and float32(uint8 / 255.0) (heatmap.py:59-61) are the same 256 numbers
    u = np.arange(256)
    assert np.array_equal(u.astype(np.float32) / np.float32(255), (u / 255.0).astype(np.float32))


def test_host_build_reproduces_the_reference_rows(golden, evalcheck):
    z = golden("eval_cases.npz")
    table = z["table"]
    full = np.concatenate([table, np.zeros((1, 3), np.uint8)])
    for key in ("ramp", "edge"):
        e = np.ascontiguousarray(z[key])
        bins = np.empty(len(e), np.int32)
        evalcheck.hc_eval_error_bins(len(e), ptr(e), ptr(bins))
        assert np.array_equal(full[bins], z[f"{key}_heat"]), key
    for name in PAIRS:                                        # compute_errors(target, fake) on the goldens
        gt, pred = z[f"{name}_gt"], z[f"{name}_pred"]
        got = _host(evalcheck, pred[None], gt[None])
        er.check_heat(got["heat"][0], gt, pred, full)
        assert abs(float(got["psnr"][0]) - float(z[f"{name}_psnr"])) <= PSNR_BAR
        assert abs(float(got["psnr"][0]) - float(er.psnr_ref(gt, pred))) <= PSNR_BAR
        # float32 in the reference's order: the very same bins as the reference's own float32 run, not only the edge rule
        assert np.array_equal(got["heat"][0], z[f"{name}_heat"]), name


@pytest.mark.parametrize("seed,B,H,W", er.GPU_CASES)
def test_gpu_case_inputs_meet_the_edge_cap_in_float32(seed, B, H, W):
    """The inputs of the GPU tests: float32 numpy in the reference's order (its own result) against the float64 oracle."""
    pred, image, alpha, boundary = er.make_frame_inputs(seed, B, H, W)
    for bg in (0.0, 1.0):
        a = alpha[:, 0:1] * (np.float32(1) - boundary.astype(np.float32))
        target = image * a + (np.float32(1) - a) * np.float32(bg)
        assert target.dtype == np.float32
        e32 = np.linalg.norm(np.moveaxis(target - pred, 1, -1), axis=-1, ord=2)
        assert e32.dtype == np.float32
        heat32 = np.moveaxis((er.jet_table_ref()[er.heat_bins(e32)].astype(np.float32) / np.float32(255)), -1, 1)
        n_open, n = er.check_heat(heat32, target, pred)
        print(f"({B},{H},{W}) bg {bg}: {n_open} of {n} pixels within {er.EDGE} of a bin edge")
        t64, _ = er.compose_ref(image, alpha, boundary, bg)
        assert float(np.abs(target - t64).max()) <= COMPOSE_BAR


@pytest.mark.parametrize("seed,B,H,W", er.GPU_CASES + [(105, 2, 3, 1500)])
def test_host_build_equals_the_oracle(evalcheck, seed, B, H, W):
    for channels in (1, 3):
        pred, image, alpha, boundary = er.make_frame_inputs(seed, B, H, W, channels)
        for bg in (0.0, 1.0):
            want_t, want_g = er.compose_ref(image, alpha, boundary, bg)
            first = None
            for bd in (boundary, boundary.astype(np.bool_), boundary.astype(np.float32)):
                got = _host(evalcheck, pred, image, alpha, bd, BG_WHITE if bg else 0)
                assert float(np.abs(got["target"] - want_t).max()) <= COMPOSE_BAR
                assert float(np.abs(got["gt"] - want_g).max()) <= COMPOSE_BAR
                er.check_heat(got["heat"], got["target"], pred)
                want_p = er.psnr_ref(got["target"], pred)
                assert float(np.abs(got["psnr"] - want_p).max()) <= PSNR_BAR
                assert float(np.abs(got["psnr_channels"] - er.psnr_channels_ref(got["target"], pred)).max()) <= PSNR_BAR
                if first is None:
                    first = got
                for k in got:                                 # the three boundary dtypes: the same bits
                    assert np.array_equal(got[k], first[k]), k
    assert evalcheck.hc_eval_partials(H, W) == -(-H * W // 4096)


def test_host_build_at_the_special_errors(evalcheck):
    gt, pred = er.make_pair(7, 9, 11)
    # e = 0 everywhere: bin 0 everywhere, an infinite PSNR and no NaN
    got = _host(evalcheck, gt[None], gt[None])
    lut = er.jet_table_ref().astype(np.float32) / np.float32(255)
    assert (np.moveaxis(got["heat"][0], 0, -1) == lut[0]).all()
    assert np.isposinf(got["psnr"]).all() and np.isposinf(got["psnr_channels"]).all()
    # one channel identical, the others not: its PSNR is +inf and so is the mean, as in torch
    half = pred.copy()
    half[1] = gt[1]
    got = _host(evalcheck, half[None], gt[None])
    assert np.isposinf(got["psnr_channels"][0, 1]) and np.isfinite(got["psnr_channels"][0, 0]) and np.isposinf(got["psnr"][0])
    # e >= 1: the last bin, from exactly 1 (one channel off by one) to far beyond; the neighbours of 1
    far = gt.copy()
    far[:, 0, 0] = gt[:, 0, 0] + 5.0
    far[:, 0, 1] = np.array([gt[0, 0, 1] + 1.0, gt[1, 0, 1], gt[2, 0, 1]])
    exact = np.zeros((1, 3, 1, 4), np.float32)
    tgt = np.zeros_like(exact)
    tgt[0, 0, 0] = [1.0, np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(1), np.float32(2)), 255.0 / 256]
    bins = np.moveaxis(_host(evalcheck, exact, tgt)["heat"][0], 0, -1)[0]
    assert (bins[0] == lut[255]).all() and (bins[1] == lut[255]).all() and (bins[2] == lut[255]).all() and (bins[3] == lut[255]).all()
    got = _host(evalcheck, far[None], gt[None])
    assert (np.moveaxis(got["heat"][0], 0, -1)[0, 0] == lut[255]).all()
    assert (np.moveaxis(got["heat"][0], 0, -1)[0, 1] == lut[255]).all()                     # e = 1 exactly
    assert (np.moveaxis(got["heat"][0], 0, -1)[1:] == lut[0]).all()
    # NaN in one channel of one pixel: the bad colour there, nowhere else; the PSNR is NaN, not an exception
    bad = pred.copy()
    bad[2, 4, 5] = np.nan
    got = _host(evalcheck, bad[None], gt[None])
    heat = np.moveaxis(got["heat"][0], 0, -1)
    assert (heat[4, 5] == 0).all() and np.isnan(got["psnr"][0]) and np.isfinite(got["psnr_channels"][0, :2]).all()
    ok = np.ones((9, 11), bool)
    ok[4, 5] = False
    want, _, _ = er.heatmap_ref(gt, pred)
    assert np.array_equal(heat[ok], np.moveaxis(want, 0, -1)[ok])


def test_host_build_of_the_ssim_tiles_meets_the_reference(golden, evalcheck):
    """eval_ssim_tile on the CPU against the reference's own ssim: the bar test_gpu_parity.py holds d3ga_ssim_fwd to."""
    evalcheck.hc_eval_ssim.restype = ctypes.c_double
    z, zl = golden("eval_cases.npz"), golden("loss_cases.npz")
    todo = [(name, z[f"{name}_pred"], z[f"{name}_gt"], float(z[f"{name}_ssim"])) for name in PAIRS]
    todo += [("loss_" + name, zl[f"{name}_pred"], zl[f"{name}_gt"], float(zl[f"{name}_ssim"])) for name in ("a", "c")]
    for name, pred, gt, want in todo:
        _, H, W = pred.shape
        got = evalcheck.hc_eval_ssim(H, W, ptr(np.ascontiguousarray(pred)), ptr(np.ascontiguousarray(gt)))
        print(f"{name} {H}x{W}: ssim {got:.8f} reference {want:.8f} off by {abs(got - want):.2e}")
        assert abs(got - want) <= 2e-6, name
    img = np.ascontiguousarray(er.make_pair(3, 5, 7)[0])      # smaller than the window, identical images: 1
    assert abs(evalcheck.hc_eval_ssim(5, 7, ptr(img), ptr(img)) - 1.0) <= 2e-6


def test_psnr_is_the_mean_of_the_channels_not_of_the_pooled_error(evalcheck):
    rng = np.random.default_rng(5)
    gt = rng.random((1, 3, 20, 24)).astype(np.float32)
    pred = gt + (np.array([0.01, 0.05, 0.25], np.float32)[None, :, None, None] * rng.standard_normal(gt.shape)).astype(np.float32)
    mean, pooled = float(er.psnr_ref(gt, pred)[0]), float(er.psnr_pooled_ref(gt, pred)[0])
    assert abs(mean - pooled) > 0.1, (mean, pooled)           # unequal channel errors: about 9 dB apart
    got = _host(evalcheck, pred, gt)
    assert abs(float(got["psnr"][0]) - mean) <= PSNR_BAR
    assert abs(float(got["psnr"][0]) - pooled) > 0.1


def test_new_abi_surface():
    from d3ga_amd import _lib
    src = open(os.path.join(ROOT, "include", "d3ga.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], capture_output=True, text=True, check=True).stdout
    for name, ret in (("d3ga_eval_frames", "int"), ("d3ga_eval_ssim", "int"), ("d3ga_eval_finish", "int"), ("d3ga_eval_partials", "int64_t"),
                      ("d3ga_eval_ssim_partials", "int64_t"), ("d3ga_eval_jet_table", "int")):
        assert name in _lib.EXPORTS
        assert re.search(r"\b%s\s+%s\s*\(" % (ret, name), src), name
        assert hasattr(_lib.lib(), name)
        assert re.search(r"\bT %s$" % name, out, flags=re.M), name            # through csrc/d3ga.map
    assert "d3ga_*" in open(os.path.join(ROOT, "d3ga_amd", "csrc", "d3ga.map")).read()
    assert _lib.ABI_VERSION == 112 and re.search(r"#define\s+D3GA_VERSION\s+112\b", src) and _lib.lib().d3ga_version() == 112
    for name, v in (("BG_WHITE", BG_WHITE), ("COMPOSED", COMPOSED), ("ALPHA3", ALPHA3), ("BOUNDARY_F32", BOUNDARY_F32), ("MAX_PARTIALS", 2048)):
        assert getattr(_lib, "EVAL_" + name) == v == int(re.search(r"#define\s+D3GA_EVAL_%s\s+(\d+)" % name, src).group(1)), name
    build = open(os.path.join(ROOT, "d3ga_amd", "csrc", "build.py")).read()
    assert "eval.hip" in build and "eval_math.h" in build
    assert len(_lib._SIGNATURES["d3ga_eval_frames"][0]) == 13 and len(_lib._SIGNATURES["d3ga_eval_finish"][0]) == 9 and \
        len(_lib._SIGNATURES["d3ga_eval_ssim"][0]) == 7
    import d3ga_amd
    for name in ("Evaluator", "compute_errors", "compute_heatmap", "error_heatmap", "psnr"):
        assert callable(getattr(d3ga_amd, name)) and name in d3ga_amd.__all__


def test_partials_per_channel():
    from d3ga_amd import _lib
    f = _lib.lib().d3ga_eval_partials
    assert f(1, 1) == 1 and f(64, 64) == 1 and f(64, 65) == 2 and f(70, 131) == 3 and f(1080, 1920) == 507
    assert f(2160, 3840) == 2025 and f(2048, 4097) == 1639 and f(8192, 8192) == 2048       # 5 passes, then 32
    assert f(0, 5) == E_SIZE and f(5, -1) == E_SIZE and f(8192, 8193) == E_SIZE
    for hw in (1, 4096, 4097, 2 ** 23, 2 ** 23 + 1, 2 ** 26):
        assert 1 <= f(1, hw) <= _lib.EVAL_MAX_PARTIALS
    g = _lib.lib().d3ga_eval_ssim_partials                    # three channels of 16 x 16 tiles
    assert g(1, 1) == 3 and g(16, 16) == 3 and g(17, 16) == 6 and g(70, 131) == 3 * 5 * 9 and g(1080, 1920) == 3 * 68 * 120
    assert g(0, 5) == E_SIZE and g(8192, 8193) == E_SIZE


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """The refusals happen before any HIP call: host buffers stand in for device memory and are never touched."""
    from d3ga_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    odd = ctypes.c_void_p(p.value + 2)
    ok = dict(B=1, H=2, W=2, flags=0, pred=p, image=p, alpha=p, boundary_fg=p, target_out=p, gt_out=p, heat_out=p, partials=p)
    call = lambda **kw: L.d3ga_eval_frames(*{**ok, **kw}.values(), None)
    for name in ("B", "H", "W"):
        assert call(**{name: 0}) == E_SIZE and call(**{name: -2}) == E_SIZE, name
    assert call(B=65536) == E_SIZE and call(H=2 ** 13, W=2 ** 13 + 1) == E_SIZE and call(H=2 ** 16, W=2 ** 16) == E_SIZE
    for name in ("pred", "image", "alpha", "boundary_fg"):
        assert call(**{name: None}) == E_NULL, name
    assert call(target_out=None, gt_out=None, heat_out=None, partials=None) == E_NULL
    assert call(flags=16) == E_CONFIG and call(flags=-1) == E_CONFIG
    assert call(flags=COMPOSED) == E_CONFIG and call(flags=COMPOSED, target_out=None) == E_CONFIG       # nothing to compose
    assert call(flags=COMPOSED, alpha=None, boundary_fg=None, target_out=None, gt_out=None, heat_out=None, partials=None) == E_NULL
    for name in ("pred", "image", "alpha", "target_out", "gt_out", "heat_out", "partials"):
        assert call(**{name: odd}) == E_CONFIG, name
    assert call(flags=BOUNDARY_F32, boundary_fg=odd) == E_CONFIG
    ssim = lambda **kw: L.d3ga_eval_ssim(*{**dict(B=1, H=2, W=2, pred=p, target=p, ssim_partials=p), **kw}.values(), None)
    for name in ("B", "H", "W"):
        assert ssim(**{name: 0}) == E_SIZE and ssim(**{name: -1}) == E_SIZE, name
    assert ssim(B=65536) == E_SIZE and ssim(H=2 ** 13, W=2 ** 13 + 1) == E_SIZE
    for name in ("pred", "target", "ssim_partials"):
        assert ssim(**{name: None}) == E_NULL and ssim(**{name: odd}) == E_CONFIG, name
    ok2 = dict(B=1, H=2, W=2, partials=p, ssim=p, metrics=p, psnr_channels=p, accum=p)
    fin = lambda **kw: L.d3ga_eval_finish(*{**ok2, **kw}.values(), None)
    for name in ("B", "H", "W"):
        assert fin(**{name: 0}) == E_SIZE and fin(**{name: -1}) == E_SIZE, name
    assert fin(B=65536) == E_SIZE and fin(H=2 ** 13, W=2 ** 13 + 1) == E_SIZE
    assert fin(partials=None) == E_NULL and fin(metrics=None, psnr_channels=None, accum=None) == E_NULL
    assert fin(ssim=None) == E_CONFIG                         # the running sums need both metrics
    for name in ("partials", "ssim", "metrics", "psnr_channels"):
        assert fin(**{name: odd}) == E_CONFIG, name
    assert fin(accum=ctypes.c_void_p(p.value + 4)) == E_CONFIG
    assert L.d3ga_eval_jet_table(None) == E_NULL
    assert not any(buf)


def test_python_layer_validates_on_the_host():
    from d3ga_amd import D3GAError, Evaluator, compute_errors, compute_heatmap, error_heatmap, psnr
    H, W = 6, 8
    img, a, bf = torch.zeros(3, H, W), torch.zeros(1, H, W), torch.zeros(1, H, W, dtype=torch.uint8)
    ev = Evaluator("white")
    bad = [
        lambda: Evaluator("grey"),                                                           # background
        lambda: Evaluator(None),
        lambda: compute_errors(img, torch.zeros(3, H, W + 1)),                               # shapes
        lambda: compute_errors(img[None], img[None]),
        lambda: compute_errors(torch.zeros(4, H, W), torch.zeros(4, H, W)),
        lambda: compute_errors(img.double(), img.double()),                                  # dtype
        lambda: compute_errors(img.numpy(), img),
        lambda: compute_heatmap(img, img.half()),
        lambda: compute_heatmap(img[None], img[None]),
        lambda: psnr(torch.zeros(1, H, W), torch.zeros(1, H, W)),
        lambda: psnr(img, img.transpose(1, 2)),
        lambda: error_heatmap(torch.zeros(3, W, H).transpose(1, 2), img),                    # contiguity
        lambda: error_heatmap(torch.zeros(2, 2, 3, H, W), torch.zeros(2, 2, 3, H, W)),
        lambda: error_heatmap(torch.zeros(3, 0, W), torch.zeros(3, 0, W)),
        lambda: ev.add(img, img, torch.zeros(2, H, W), bf),                                  # alpha channels
        lambda: ev.add(img, img, a.double(), bf),
        lambda: ev.add(img, img, a[None], bf),                                               # batched alpha, single frame
        lambda: ev.add(img[None], img[None], a, bf),
        lambda: ev.add(img, img, a, bf.int()),                                               # boundary dtype
        lambda: ev.add(img, img, a, torch.zeros(2, H, W, dtype=torch.uint8)),                # boundary elements
        lambda: ev.add(img, img, a, torch.zeros(W, H, dtype=torch.uint8)),
        lambda: ev.add(img, img, a, None),
        lambda: ev.add(img, img.to("meta"), a, bf),                                          # device
        lambda: ev.add(torch.zeros(2, 3, H, W), torch.zeros(2, 3, H, W), torch.zeros(3, 1, H, W), torch.zeros(2, 1, H, W)),
    ]
    for i, fn in enumerate(bad):
        with pytest.raises(ValueError):
            fn()
            pytest.fail(f"case {i} was accepted")
    # everything fits, but the tensors live on the CPU: require_cuda's refusal, a ValueError and a D3GAError at once
    for fn in (lambda: compute_errors(img, img), lambda: compute_heatmap(img, img), lambda: psnr(img, img),
               lambda: error_heatmap(img, img), lambda: ev.add(img, img, a, bf), lambda: ev.add(img, img, a, bf[0])):
        with pytest.raises(ValueError) as info:
            fn()
        assert isinstance(info.value, D3GAError) and "GPU only" in str(info.value)
    assert ev.summary() == {"ssim": pytest.approx(float("nan"), nan_ok=True), "psnr": pytest.approx(float("nan"), nan_ok=True),
                            "lpips": pytest.approx(float("nan"), nan_ok=True), "count": 0}


def test_evaluator_writes_the_reference_line(tmp_path):
    from d3ga_amd import Evaluator
    path = tmp_path / "errors_test.txt"
    ev = Evaluator("black")
    assert ev.write(path)["count"] == 0 and not path.exists()             # test.py:200: nothing before the first frame
    ev._acc = torch.tensor([3 * 0.912345678, 3 * 31.00000449, 3.0, 0.0], dtype=torch.float64)      # three frames' sums
    m = ev.write(path)
    assert m["count"] == 3 and abs(m["ssim"] - 0.912345678) < 1e-12 and abs(m["psnr"] - 31.00000449) < 1e-12
    assert path.read_text() == "SSIM: 0.91235, PSNR: 31.00000, LPIPS: nan\n"
    ev = Evaluator("white", lpips=lambda fake, target: torch.zeros(()))
    ev._acc = torch.tensor([1.0, 59.999996, 2.0, 0.25], dtype=torch.float64)
    ev.write(path)
    assert path.read_text() == "SSIM: 0.50000, PSNR: 30.00000, LPIPS: 0.12500\n"
    assert path.read_text() == "SSIM: %.5f, PSNR: %.5f, LPIPS: %.5f\n" % (0.5, 59.999996 / 2, 0.125)
    ev.reset()
    assert ev.summary()["count"] == 0
