"""numpy oracle of sample preparation (d3ga_amd/sample_prep.py, csrc/sample_prep_math.h), written from the rules
and not from the kernel: whole-array expressions, a padded array for the 3 x 3 window, a lookup in the order of the rules.

ActorsHQ mode (the loader's lines datasets/actorshq_dataset.py:244-276 and get_boundary_mask :201-217 restated):
    t = 0 / 1 / 128 for m < / > / == 128;  er, di = min / max of t over the in-image part of the 3 x 3 window;
    boundary = (uint8(di - er) == 1) | (5 < m < 250);  fg = (t == 1);
    label = 0 without fg, else by (r, g, b) of the part image, (0, 0, 0) read as (127, 127, 127): r 255 -> 1, g 255 -> 2,
    b 255 -> 3, r 127 -> 4, the last match winning.
Goliath mode (datasets/goliath_dataset.py:454-481): the 2 x 2 mean of the image, of the part labels and of (parts != 0);
boundary = 1 - that; an odd last row or column is dropped."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def threshold(m):
    m = np.asarray(m, np.uint8)
    return np.where(m < 128, 0, np.where(m > 128, 1, 128)).astype(np.uint8)


def window_min_max(t):
    """(H,W) uint8 -> (min, max) over the in-image part of the 3 x 3 window: the border is padded with the neutral value"""
    H, W = t.shape
    lo = np.pad(t, 1, constant_values=255)
    hi = np.pad(t, 1, constant_values=0)
    shifts = [(dy, dx) for dy in range(3) for dx in range(3)]
    er = np.min([lo[dy:dy + H, dx:dx + W] for dy, dx in shifts], axis=0)
    di = np.max([hi[dy:dy + H, dx:dx + W] for dy, dx in shifts], axis=0)
    return er.astype(np.uint8), di.astype(np.uint8)


def boundary_and_fg(m):
    """(H,W) uint8 matte -> (boundary, fg) bool"""
    m = np.asarray(m, np.uint8)
    t = threshold(m)
    er, di = window_min_max(t)
    return ((di - er).astype(np.uint8) == 1) | ((m > 5) & (m < 250)), t == 1


def labels(seg_bgr, fg):
    """(H,W,3) uint8 BGR part image, (H,W) bool -> (H,W) int32"""
    rgb = np.asarray(seg_bgr)[..., ::-1].astype(np.int64)
    rgb = np.where(rgb.sum(-1, keepdims=True) == 0, 127, rgb)
    out = np.zeros(fg.shape, np.int32)
    for value, (channel, level) in enumerate(((0, 255), (1, 255), (2, 255), (0, 127)), start=1):
        out[rgb[..., channel] == level] = value
    return np.where(fg, out, 0).astype(np.int32)


def actorshq_ref(image_bgr, seg_bgr, mask, image_dtype=np.uint8):
    """image (B,H,W,3), seg (B,Hs,Ws,3), mask (B,H,W) uint8 -> dict: image (B,3,H,W) RGB of image_dtype, seg_part (B,1,H,W)
    int32, seg_fg and boundary_fg (B,1,H,W) float32"""
    image_bgr, seg_bgr, mask = (np.asarray(a, np.uint8) for a in (image_bgr, seg_bgr, mask))
    B, H, W, _ = image_bgr.shape
    pairs = [boundary_and_fg(mask[b]) for b in range(B)]
    boundary, fg = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    part = np.stack([labels(seg_bgr[b, :H, :W], fg[b]) for b in range(B)])
    return {"image": np.ascontiguousarray(image_bgr[..., ::-1].transpose(0, 3, 1, 2)).astype(image_dtype),
            "seg_part": part[:, None], "seg_fg": fg[:, None].astype(np.float32), "boundary_fg": boundary[:, None].astype(np.float32)}


def half(x):
    """(..., H, W) -> (..., H // 2, W // 2) float32: the mean of each 2 x 2 block, in float64 and exact"""
    x = np.asarray(x, np.float64)
    oh, ow = x.shape[-2] // 2, x.shape[-1] // 2
    x = x[..., :2 * oh, :2 * ow].reshape(x.shape[:-2] + (oh, 2, ow, 2))
    return x.mean(axis=(-3, -1)).astype(np.float32)


def goliath_ref(image, parts):
    """image (B,3,H,W), parts (B,1,H,W) uint8 -> dict of float32 (B,3|1|1|1,H//2,W//2)"""
    fg = half(np.asarray(parts) != 0)
    return {"image": half(image), "seg_part": half(parts), "seg_fg": fg, "boundary_fg": (1.0 - fg.astype(np.float64)).astype(np.float32)}


def random_actorshq(seed, B, H, W, extra=(0, 0)):
    """Inputs that reach every rule at any size: a blocky matte with soft values, 128s and the rule's thresholds sprinkled in;
    part colours from the palette the rules name plus noise, black and a native red of 127."""
    rng = np.random.default_rng(seed)
    Hs, Ws = H + extra[0], W + extra[1]
    image = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    coarse = rng.random((B, H // 4 + 1, W // 4 + 1)) < 0.5
    mask = np.where(np.kron(coarse, np.ones((4, 4), bool))[:, :H, :W], 255, 0).astype(np.uint8)
    special = np.array([0, 5, 6, 127, 128, 129, 249, 250, 255, 128, 128, 1, 200], np.uint8)
    pick = rng.random((B, H, W)) < 0.3
    mask[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    palette = np.array([[0, 0, 255], [0, 255, 0], [255, 0, 0], [127, 127, 127], [0, 0, 0], [9, 200, 127], [255, 255, 255], [255, 0, 127],
                        [0, 255, 255], [3, 4, 5], [127, 255, 255]], np.uint8)           # BGR
    seg = palette[rng.integers(0, len(palette), (B, Hs, Ws))]
    noise = rng.random((B, Hs, Ws)) < 0.1
    seg[noise] = rng.integers(0, 256, (int(noise.sum()), 3), dtype=np.uint8)
    return image, seg, mask


def random_goliath(seed, B, H, W):
    rng = np.random.default_rng(seed)
    image = rng.integers(0, 256, (B, 3, H, W), dtype=np.uint8)
    parts = np.where(rng.random((B, 1, H, W)) < 0.5, rng.integers(1, 256, (B, 1, H, W)), 0).astype(np.uint8)
    return image, parts


# ---- the g++ build of csrc/sample_prep_math.h -------------------------------------------------------------------------------------
_LIB = []


def lib():
    if not _LIB:
        src = os.path.join(ROOT, "tests", "hostcheck", "sample_prep_host.cpp")
        out_dir = os.path.join(ROOT, "tests", "hostcheck", "_build")
        os.makedirs(out_dir, exist_ok=True)
        so = os.path.join(out_dir, "libsample_prep_host.so")
        deps = [src, os.path.join(ROOT, "include", "d3ga.h"), os.path.join(ROOT, "d3ga_amd", "csrc", "sample_prep_math.h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", so])
        L = ctypes.CDLL(so)
        i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
        L.hc_sample_prep_actorshq.argtypes = [i32] * 5 + [vp, i64, i64] * 3 + [i32, i32] + [vp] * 4 + [ctypes.POINTER(i32), i32]
        L.hc_sample_prep_goliath.argtypes = [i32] * 3 + [vp, i64, i64, i64, vp, i64, i64] + [vp] * 4 + [ctypes.POINTER(i32)]
        _LIB.append(L)
    return _LIB[0]


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


NAMES = ("image", "seg_part", "seg_fg", "boundary_fg")


def host_actorshq(image, seg, mask, image_dtype=np.uint8, force_scalar=False, skip=()):
    """The g++ build on numpy arrays (B,H,W,3), (B,Hs,Ws,3), (B,H,W): views are addressed through their strides, as the Python
    layer addresses tensors.  -> (dict of outputs, path); an output named in `skip` is passed as NULL and comes back as None."""
    B, H, W, _ = image.shape
    Hs, Ws = seg.shape[1:3]
    out = {"image": np.zeros((B, 3, H, W), image_dtype), "seg_part": np.full((B, 1, H, W), -9, np.int32),
           "seg_fg": np.full((B, 1, H, W), np.nan, np.float32), "boundary_fg": np.full((B, 1, H, W), np.nan, np.float32)}
    for n in skip:
        out[n] = None
    path = ctypes.c_int32(-1)
    st = lib().hc_sample_prep_actorshq(B, H, W, Hs, Ws, _p(image), image.strides[1], image.strides[0], _p(seg), seg.strides[1], seg.strides[0],
                                       _p(mask), mask.strides[1], mask.strides[0], mask.strides[2], int(np.dtype(image_dtype) == np.float32),
                                       *[_p(out[n]) for n in NAMES], ctypes.byref(path), int(force_scalar))
    assert st == 0, st
    return out, path.value


def host_goliath(image, parts, skip=()):
    B, _, H, W = image.shape
    out = {n: np.full((B, 3 if n == "image" else 1, H // 2, W // 2), np.nan, np.float32) for n in NAMES}
    for n in skip:
        out[n] = None
    path = ctypes.c_int32(-1)
    st = lib().hc_sample_prep_goliath(B, H, W, _p(image), image.strides[2], image.strides[1], image.strides[0], _p(parts), parts.strides[2],
                                      parts.strides[0], *[_p(out[n]) for n in NAMES], ctypes.byref(path))
    assert st == 0, st
    return out, path.value
