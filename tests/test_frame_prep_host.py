"""Frame preparation without a GPU: the numpy oracle (tests/frame_ref.py) against the reference's own linear2color_corr and
Batcher.get_silhouette (tests/golden/frame_cases.npz, tools/gen_golden.py: gen_frames); the CPU build of
csrc/frame_prep_math.h -- the text the kernel runs -- against the oracle; the majority rule against the sorted median; the
colour table's precedence; the ABI surface and its refusals; the Python layer's ValueErrors."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import frame_ref as fr
from conftest import ROOT, ptr

E_NULL, E_SIZE, E_CONFIG = -1, -2, -3            # D3GA_E_* (include/d3ga.h)
GAMMA, BG_WHITE, ERODE_MASK, CLOSE_HOLES, IMAGE_U8, SEG_F32 = 1, 2, 4, 8, 16, 32
# |a - b| <= 1e-6, derived (not measured): six correctly rounded float32 operations on values <= 2 (2^-24 relative each); behind
# the output clamp, which removes the steep part of the square root, the slope against the input is at most k / (2 * 0.0588),
# about 8.2, where the input is about 0.015 -- 8.2 * 3 * 2^-24 * 0.015 plus 3 * 2^-24 * 2 stays below 4e-7
COLOR_BAR = 1e-6
GOLIATH = {"body": {"label_id": [1]}, "upper": {"label_id": [27]}, "lower": {"label_id": [16]}}


@pytest.fixture(scope="module")
def framecheck():
    src = os.path.join(ROOT, "tests", "hostcheck", "frame_prep_host.cpp")
    out_dir = os.path.join(ROOT, "tests", "hostcheck", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libframe_prep_host.so")
    deps = [src, os.path.join(ROOT, "d3ga_amd", "csrc", "frame_prep_math.h"), os.path.join(ROOT, "include", "d3ga.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", so])
    return ctypes.CDLL(so)


def _cages(z, name):
    return {k: {"label_id": [int(v) for v in ids.split(",")]} for k, ids in (str(s).split(":") for s in z[f"cages_{name}"])}


def _table(cages, background):
    from d3ga_amd.frame_prep import silhouette_table
    t, o, bg = silhouette_table(cages, background)
    return np.ascontiguousarray(t.numpy()), np.ascontiguousarray(o.numpy()), bg


def _host(lib, image, seg_part, seg_fg, cages, flags, outputs=("image", "orig_image", "alpha", "silhouette")):
    """hc_frame_prep (the kernel's tile loop on the CPU) -> dict of float32 arrays."""
    B, _, H, W = image.shape
    t, o, bg = _table(cages, "white" if flags & BG_WHITE else "black")
    image = np.ascontiguousarray(image, dtype=np.uint8 if flags & IMAGE_U8 else np.float32)
    seg_part = np.ascontiguousarray(seg_part, dtype=np.float32 if flags & SEG_F32 else np.int32)
    seg_fg = None if seg_fg is None else np.ascontiguousarray(seg_fg, dtype=np.float32)
    out = {n: np.full((B, 1 if n == "alpha" else 3, H, W), np.nan, np.float32) for n in outputs}
    assert lib.hc_frame_prep(B, H, W, flags, ptr(image), ptr(seg_part), ptr(seg_fg), ptr(t), t.shape[0], ptr(o), ptr(out.get("image")),
                             ptr(out.get("orig_image")), ptr(out.get("alpha")), ptr(out.get("silhouette"))) == 0
    return out


def _inputs(rng, B, H, W, n_labels=30, density=0.5):
    image = rng.integers(0, 256, (B, 3, H, W)).astype(np.float32)
    seg_part = np.where(rng.random((B, 1, H, W)) < density, rng.integers(1, n_labels, (B, 1, H, W)), 0).astype(np.int32)
    seg_fg = (rng.random((B, 1, H, W)) < 0.2).astype(np.float32)
    return image, seg_part, seg_fg


def test_oracle_equals_the_reference(golden):
    z = golden("frame_cases.npz")
    got = fr.linear2color_ref(z["color_in"] / 255.0, 0)
    assert z["color_in"].shape == (3, 24, 40) and z["color_in"].dtype == np.float64
    for c in range(3):                                        # the black clamp bites at the integers 0..8: all of them are there
        assert set(range(256)) <= set(z["color_in"][c].ravel().tolist())
    assert float(np.abs(got - z["color_out"]).max()) <= 1e-12
    assert (z["color_out"] == 0).any() and float(z["color_out"].max()) > 1.0
    seg = z["sil_seg"]
    assert set(range(31)) <= set(seg.ravel().tolist())
    names = [str(s) for s in z["sil_sets"]]
    assert names == ["body", "body_face", "goliath", "shared", "absent"]
    for name in names:
        cages = _cages(z, name)
        for bg in ("white", "black"):
            want = z[f"sil_{name}_{bg}"]
            assert np.array_equal(fr.silhouette_ref(seg[0], cages, bg), want), (name, bg)
            # ... and the colour table of the Python layer, looked up the way the kernel does
            t, o, v = _table(cages, bg)
            s = seg[0].astype(np.int64)
            idx = np.where(s == 0, 0, np.where((s > 0) & (s < len(t)), s, len(t)))
            lut = np.concatenate([t, o[None]]).astype(np.float64)
            lut[0] = v
            assert np.array_equal(np.moveaxis(lut[idx], -1, 0), want), (name, bg)


def test_host_build_of_the_colour_math_meets_the_derived_bar(framecheck):
    rng = np.random.default_rng(7)
    v = np.concatenate([np.arange(256.0), np.arange(0.0, 12.0, 1.0 / 64), rng.uniform(0.0, 255.0, 20000)]).astype(np.float32)
    worst = 0.0
    for gamma in (0, 1):
        for c in range(3):
            out = np.empty_like(v)
            framecheck.hc_frame_orig(len(v), ptr(v), c, gamma, ptr(out))
            x = v.astype(np.float64) / 255.0
            img = np.zeros((3, len(v)))
            img[c] = x
            want = fr.linear2color_ref(img, 0)[c] if gamma else x
            worst = max(worst, float(np.abs(out - want).max()))
    print(f"frame_orig host build: worst |a - b| = {worst:.3e} = {worst / COLOR_BAR:.3f} of the bar")
    assert worst <= COLOR_BAR


@pytest.mark.parametrize("H,W,B", [(1, 1, 1), (3, 5, 1), (1, 9, 1), (17, 63, 1), (33, 64, 1), (3, 65, 2), (70, 130, 1), (33, 5, 3)])
def test_host_build_equals_the_oracle(framecheck, H, W, B):
    rng = np.random.default_rng(H * 1000 + W)
    image, seg_part, seg_fg = _inputs(rng, B, H, W)
    seg_part[0, 0, 0, 0] = -3                                 # a negative label: no foreground, "other" colour
    seg_part[-1, 0, -1, -1] = 77                              # a label behind the table
    for flags in (0, GAMMA | BG_WHITE, ERODE_MASK, CLOSE_HOLES | BG_WHITE, GAMMA | ERODE_MASK | CLOSE_HOLES, IMAGE_U8 | BG_WHITE | ERODE_MASK):
        got = _host(framecheck, image, seg_part, seg_fg, GOLIATH, flags)
        want = fr.frame_ref(image, seg_part, seg_fg, GOLIATH, bool(flags & GAMMA), "white" if flags & BG_WHITE else "black",
                            bool(flags & ERODE_MASK), bool(flags & CLOSE_HOLES))
        assert np.array_equal(got["alpha"], want["alpha"]), flags
        assert np.array_equal(got["silhouette"], want["silhouette"]), flags
        assert float(np.abs(got["orig_image"] - want["orig_image"]).max()) <= COLOR_BAR
        bgv = np.float32(1.0 if flags & BG_WHITE else 0.0)
        assert np.array_equal(got["image"], np.where(want["fg"], got["orig_image"], bgv)), flags     # the fg selection: exact
    # float labels truncate as .int() does; without seg_fg the labels alone decide
    segf = seg_part.astype(np.float32) + np.where(seg_part >= 0, 0.9, -0.9).astype(np.float32)
    segf[0, 0, 0, -1] = 0.5
    got = _host(framecheck, image, segf, None, GOLIATH, SEG_F32 | BG_WHITE)
    want = fr.frame_ref(image, segf, None, GOLIATH, False, "white")
    assert np.array_equal(fr.labels_ref(segf), np.where(segf == 0.5, 0, seg_part))
    for k in ("alpha", "silhouette"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["image"], np.where(want["fg"], got["orig_image"], np.float32(1)))


def _median_cases():
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:23, 0:70]
    cases = {"checkerboard": ((yy + xx) % 2).astype(np.float32), "ones": np.ones((20, 21), np.float32)}
    for d in (0.3, 0.5, 0.7):
        cases[f"random{d}"] = (rng.random((37, 71)) < d).astype(np.float32)
    for hw in ((3, 5), (1, 1), (1, 9)):
        cases["small%dx%d" % hw] = np.ones(hw, np.float32)
        cases["small%dx%dr" % hw] = (rng.random(hw) < 0.6).astype(np.float32)
    return cases


@pytest.mark.parametrize("name", list(_median_cases()))
def test_majority_rule_equals_the_sorted_median(framecheck, name):
    m = _median_cases()[name]
    H, W = m.shape
    got = _host(framecheck, np.zeros((1, 3, H, W)), np.zeros((1, 1, H, W)), m[None, None], GOLIATH, 0, outputs=("alpha",))["alpha"][0, 0]
    want = fr.median_ref(m)
    assert np.array_equal(got, want)
    if name == "checkerboard":                                # interior counts are 24 or 25 by parity
        assert got[3:-3, 3:-3].min() == 0 and got[3:-3, 3:-3].max() == 1
        assert np.array_equal(got[3:-3, 3:-3], m[3:-3, 3:-3])
    if name == "ones":                                        # corner 4 * 4 = 16 -> 0; row 0: col 2 4 * 6 = 24 -> 0, col 3 4 * 7 = 28 -> 1
        assert got[0, 0] == 0 and got[0, 2] == 0 and got[0, 3] == 1 and got[3, 3] == 1
    if name.startswith("small"):
        assert not got.any()                                  # at most 15 ones in a window: never a majority of 49


def test_morphology_reads_the_image_border_as_the_rules_say(framecheck):
    """One foreground block against the image corner, sized so that the median keeps it: a dilation must not leak in from
    outside (outside reads as 0) and an erosion must not eat the border (outside reads as 1)."""
    m = np.zeros((40, 50), np.float32)
    m[:20, :24] = 1
    m[30:, 44:] = 1
    for flags in (ERODE_MASK, CLOSE_HOLES, ERODE_MASK | CLOSE_HOLES):
        got = _host(framecheck, np.zeros((1, 3, 40, 50)), np.zeros((1, 1, 40, 50)), m[None, None], GOLIATH, flags, outputs=("alpha",))["alpha"][0, 0]
        want = fr.alpha_ref(m, bool(flags & ERODE_MASK), bool(flags & CLOSE_HOLES))
        assert np.array_equal(got, want), flags
        assert got[0, 0] == 1 and got[-1, -1] == 1 and got[0, -1] == 0
    a = fr.alpha_ref(m, True, False)
    assert a[10, 24] == 1 and a[10, 25] == 0 and fr.alpha_ref(m)[10, 24] == 0      # dilate 7, erode 5: a straight edge grows by one pixel


def test_silhouette_table_precedence_and_the_body_only_case():
    from d3ga_amd.frame_prep import BLUE, GRAY, GREEN, RED, silhouette_table
    t, o, bg = silhouette_table({"upper": {"label_id": [4, 5]}, "lower": {"label_id": [5, 6]}, "face": {"label_id": [6, -1, 2]}}, "white")
    assert bg == 1.0 and tuple(o.tolist()) == BLUE and t.shape == (7, 3) and t.dtype == torch.float32
    rows = {i: tuple(t[i].tolist()) for i in range(7)}
    assert rows[4] == RED and rows[5] == GREEN and rows[6] == GRAY and rows[2] == GRAY      # later wins: lower over upper, face over lower
    assert rows[1] == BLUE and rows[3] == BLUE and rows[0] == (1.0, 1.0, 1.0)
    # objects with an attribute, black background, a label absent from every list
    ns = lambda ids: type("Cage", (), {"label_id": ids})()
    t, o, bg = silhouette_table({"body": ns([1]), "upper": ns([27]), "lower": ns([16])}, "Black")
    assert bg == 0.0 and t.shape == (28, 3) and tuple(t[27].tolist()) == RED and tuple(t[16].tolist()) == GREEN
    assert tuple(t[1].tolist()) == BLUE and tuple(t[0].tolist()) == (0.0, 0.0, 0.0)
    # {body} and {body, face}: nothing red, green or gray; the face labels keep the background
    for bgname, v in (("white", 1.0), ("black", 0.0)):
        t, o, bg = silhouette_table({"body": {"label_id": [1]}, "face": {"label_id": [3, 9]}}, bgname)
        assert t.shape == (10, 3) and tuple(t[3].tolist()) == tuple(t[9].tolist()) == (v, v, v) and tuple(t[1].tolist()) == BLUE
        t, o, bg = silhouette_table({"body": {"label_id": [1]}}, bgname)
        assert t.shape == (1, 3) and tuple(o.tolist()) == BLUE
    # three cages with body and face: the general rule again
    t, _, _ = silhouette_table({"body": {"label_id": [1]}, "face": {"label_id": [3]}, "upper": {"label_id": [2]}}, "white")
    assert tuple(t[3].tolist()) == GRAY and tuple(t[2].tolist()) == RED
    with pytest.raises(ValueError):
        silhouette_table({"upper": {"label_id": [0]}}, "white")
    with pytest.raises(ValueError):
        silhouette_table({"upper": {"label_id": [-2]}}, "white")
    with pytest.raises(ValueError):
        silhouette_table({"upper": {}}, "white")


def test_frame_prep_reads_the_batcher_configuration():
    from d3ga_amd.frame_prep import FramePrep
    cfg = {"train": {"erode_mask": True, "use_gamma_space": True, "background": "Black"}, "cages": GOLIATH}
    p = FramePrep(cfg)
    assert (p.erode_mask, p.close_holes, p.gamma, p.background) == (True, False, True, "black")
    ns = lambda **k: type("Node", (), k)()
    p = FramePrep(ns(train=ns(use_close_holes=True), cages=GOLIATH))
    assert (p.erode_mask, p.close_holes, p.gamma, p.background) == (False, True, False, "white")
    assert p.table("cpu")[0].shape == (28, 3) and p.table("cpu") is p.table("cpu")


def test_new_abi_surface():
    from d3ga_amd import _lib
    src = open(os.path.join(ROOT, "include", "d3ga.h")).read()
    assert "d3ga_frame_prep" in _lib.EXPORTS
    assert re.search(r"\bint\s+d3ga_frame_prep\s*\(", src)
    assert hasattr(_lib.lib(), "d3ga_frame_prep")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT d3ga_frame_prep$", out, flags=re.M)                 # through csrc/d3ga.map
    assert "d3ga_*" in open(os.path.join(ROOT, "d3ga_amd", "csrc", "d3ga.map")).read()
    assert _lib.ABI_VERSION == 112 and re.search(r"#define\s+D3GA_VERSION\s+112\b", src) and _lib.lib().d3ga_version() == 112
    for name in ("GAMMA", "BG_WHITE", "ERODE_MASK", "CLOSE_HOLES", "IMAGE_U8", "SEG_F32"):
        assert getattr(_lib, "FRAME_" + name) == int(re.search(r"#define\s+D3GA_FRAME_%s\s+(\d+)" % name, src).group(1)), name
    assert (GAMMA, BG_WHITE, ERODE_MASK, CLOSE_HOLES, IMAGE_U8, SEG_F32) == tuple(getattr(_lib, "FRAME_" + n) for n in
                                                                                  ("GAMMA", "BG_WHITE", "ERODE_MASK", "CLOSE_HOLES", "IMAGE_U8", "SEG_F32"))
    assert "frame_prep.hip" in open(os.path.join(ROOT, "d3ga_amd", "csrc", "build.py")).read()
    assert len(_lib._SIGNATURES["d3ga_frame_prep"][0]) == 15


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """The refusals happen before any HIP call: host buffers stand in for device memory and are never touched."""
    from d3ga_amd import _lib
    f = _lib.lib().d3ga_frame_prep
    buf = (ctypes.c_float * 64)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    odd = ctypes.c_void_p(p.value + 4)
    ok = dict(B=1, H=4, W=4, flags=0, image=p, seg_part=p, seg_fg=p, label_rgb=p, n_labels=2, other_rgb=p, image_out=p, orig_out=p,
              alpha_out=p, sil_out=p)
    call = lambda **kw: f(*{**ok, **kw}.values(), None)
    for name in ("B", "H", "W"):
        assert call(**{name: 0}) == E_SIZE and call(**{name: -2}) == E_SIZE, name
    assert call(n_labels=0) == E_SIZE and call(n_labels=-1) == E_SIZE
    assert call(B=65536) == E_SIZE and call(H=2 ** 16, W=2 ** 15) == E_SIZE
    for name in ("image", "seg_part", "label_rgb", "other_rgb"):
        assert call(**{name: None}) == E_NULL, name
    assert call(image_out=None, orig_out=None, alpha_out=None, sil_out=None) == E_NULL
    assert call(flags=64) == E_CONFIG and call(flags=-1) == E_CONFIG
    for name in ("image", "image_out", "orig_out", "alpha_out", "sil_out"):
        assert call(**{name: odd}) == E_CONFIG, name
    assert not any(buf)


def test_python_layer_validates_on_the_host():
    from d3ga_amd import _lib
    from d3ga_amd.frame_prep import prepare_frames, silhouette_table
    table = silhouette_table(GOLIATH, "white")
    B, H, W = 2, 6, 8
    img, seg, sfg = torch.zeros(B, 3, H, W), torch.zeros(B, 1, H, W, dtype=torch.int32), torch.zeros(B, 1, H, W)
    kw = dict(table=table, gamma=True)
    bad = [
        lambda: prepare_frames(img[0], seg, sfg, **kw),                                       # not (B,3,H,W)
        lambda: prepare_frames(torch.zeros(B, 4, H, W), seg, sfg, **kw),
        lambda: prepare_frames(img.double(), seg, sfg, **kw),                                 # dtype
        lambda: prepare_frames(img, seg.long(), sfg, **kw),
        lambda: prepare_frames(img, seg, sfg.double(), **kw),
        lambda: prepare_frames(img, seg[:, :, :-1], sfg, **kw),                               # shape
        lambda: prepare_frames(img, seg, sfg[:1], **kw),
        lambda: prepare_frames(torch.zeros(B, 3, W, H).transpose(2, 3), seg, sfg, **kw),      # contiguity
        lambda: prepare_frames(torch.zeros(B * 3 * H * W + 1)[1:].view(B, 3, H, W), seg, sfg, **kw),       # alignment
        lambda: prepare_frames(img, seg, sfg, table=table[:2], gamma=True),
        lambda: prepare_frames(img, seg, sfg, table=(table[0][:, :2], table[1], table[2]), gamma=True),
        lambda: prepare_frames(img, seg, sfg, background="black", **kw),                      # the table is white
        lambda: prepare_frames(img, seg, sfg, out={"alpha": torch.zeros(B, 3, H, W)}, **kw),
        lambda: prepare_frames(img, seg, sfg, out={"image": torch.zeros(B, 3, H, W, dtype=torch.float64)}, **kw),
        lambda: prepare_frames(img, seg, sfg, out={"mask": torch.zeros(B, 1, H, W)}, **kw),
        lambda: prepare_frames(img, seg, sfg, out={"silhouette": torch.zeros(B, 3, H, W, device="meta")}, **kw),     # device
    ]
    for i, fn in enumerate(bad):
        with pytest.raises(ValueError):
            fn()
            pytest.fail(f"case {i} was accepted")
    with pytest.raises(_lib.D3GAError):                       # everything fits, but the tensors live on the CPU: no fallback
        prepare_frames(img, seg, sfg, **kw)
