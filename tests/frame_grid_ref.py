"""The frame grid (d3ga_amd/frame_grid.py) restated independently in numpy, and the g++ build of
csrc/frame_grid_math.h (tests/hostcheck/gridcheck.cpp) -- the text the kernels run -- behind ctypes."""
import ctypes
import os
import subprocess

import numpy as np
import torch

from conftest import ROOT

# |header - float64 restatement| of a blended pixel, inputs and colour in [0, 1] (DESIGN.md 4.4o has the derivation):
# coverage 3 * 2^-24 (six roundings of at most 2^-25 each), times |colour - x| <= 1; the blend adds the roundings of 1 - a, of the
# two products (2^-25 each) and of the sum (2^-24 below 2): 3 + 0.5 + 0.5 + 0.5 + 1 = 5.5, stated as 6
BLEND_BOUND = 6.0 * 2.0 ** -24
ALPHA_BOUND = 3.0 * 2.0 ** -24
MAX_UNIT = np.float32(17.7)
SLOT = b"{:.3f}"


# ---- the g++ build ------------------------------------------------------------------------------------------------------------
def gridcheck():
    src = os.path.join(ROOT, "tests", "hostcheck", "gridcheck.cpp")
    out_dir = os.path.join(ROOT, "tests", "hostcheck", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libgridcheck.so")
    deps = [src, os.path.join(ROOT, "include", "d3ga.h")] + [os.path.join(ROOT, "d3ga_amd", "csrc", h)
                                                             for h in ("frame_grid_math.h", "frame_grid_font.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", so])
    lib = ctypes.CDLL(so)
    lib.hc_grid_unit.restype = ctypes.c_float
    lib.hc_grid_unit.argtypes = [ctypes.c_int]
    lib.hc_grid_baseline.argtypes = [ctypes.c_float, ctypes.c_int, ctypes.c_int]
    lib.hc_grid_blend.restype = ctypes.c_float
    lib.hc_grid_blend.argtypes = [ctypes.c_float] * 3
    lib.hc_grid_format.argtypes = [ctypes.c_float, ctypes.c_char_p]
    lib.hc_grid_quant.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    return lib


_LIB = []


def lib():
    if not _LIB:
        _LIB.append(gridcheck())
    return _LIB[0]


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_quant(mode, x):
    from d3ga_amd import _lib
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty(x.shape, np.uint8)
    lib().hc_grid_quant({"save_image": _lib.GRID_OUT_U8_SAVE_IMAGE, "clip": _lib.GRID_OUT_U8_CLIP}[mode], _p(x), x.size, _p(out))
    return out


def host_format(x):
    buf = ctypes.create_string_buffer(32)
    n = lib().hc_grid_format(float(np.float32(x)), buf)
    return buf.raw[:n].decode()


def host_font():
    out = np.zeros((95, 7), np.uint8)
    lib().hc_grid_font(_p(out))
    return out


def cpu_panel(p):
    """A Panel over host copies of a Panel's tensors (same label, colour, flags)."""
    from d3ga_amd.frame_grid import Panel
    q = Panel(p.img.detach().cpu(), layout=p.layout)
    q.label, q.color, q.flags, q.X = p.label, p.color, p.flags, p.X
    q.value = None if p.value is None else p.value.detach().cpu()
    return q


def host_compose(placed, out_size, quantize="save_image", order="rgb", channels=3, pad_value=1.0, out_layout="chw", pitch=None):
    """d3ga_amd.frame_grid.compose_panels on the CPU: the Python layer's own descriptor over host copies of the panels, run by
    the g++ build of the header -> (numpy output, path).  Bytes beyond a padded row's pixels stay 0xAB."""
    from d3ga_amd import _lib, frame_grid as fg
    placed = [(cpu_panel(p), y0, x0) for p, y0, x0 in placed]
    h, w = out_size
    mode = fg._MODES[quantize]
    if mode is None:
        mode = _lib.GRID_OUT_F32_CHW if out_layout == "chw" else _lib.GRID_OUT_F32_HWC
        out = np.full((channels, h, w) if out_layout == "chw" else (h, w, channels), np.nan, np.float32)
        pitch = 0
    else:
        pitch = pitch or w * channels
        out = np.full((h, pitch), 0xAB, np.uint8)
    d = fg._pack(placed, h, w, mode, channels, order, pad_value, pitch)
    path = ctypes.c_int32(-1)
    st = lib().hc_grid_compose(ctypes.byref(d), _p(out), ctypes.byref(path))
    assert st == 0, st
    if mode >= _lib.GRID_OUT_U8_SAVE_IMAGE:
        out = out[:, :w * channels].reshape(h, w, channels)
    return out, path.value


def host_compose_rows(rows, pad_even=True, **kw):
    from d3ga_amd import frame_grid as fg
    placed, h, w = fg._layout_rows(rows, pad_even)
    return host_compose(placed, (h, w), **kw)[0]


def host_write_text(img, text, **kw):
    """The header's write_text of a (C,H,W) tensor -> float32 torch tensor (3 | 4, H, W)"""
    from d3ga_amd.frame_grid import Panel
    p = Panel(img.detach().cpu(), label=text, **kw)
    return torch.from_numpy(host_compose([(p, 0, 0)], (p.h, p.w), quantize=None, channels=4 if p.C == 4 else 3)[0])


def host_alpha(label, w, h, value=None, bottom=False, thickness=2, X=15):
    """coverage (h, w) float32 of a label by the header"""
    from d3ga_amd import _lib
    from d3ga_amd.frame_grid import Panel, _pack
    img = torch.zeros(1, h, w)
    cell = None if value is None else torch.tensor([value], dtype=torch.float32)
    p = Panel(img, label=label, value=cell, bottom=bottom, thickness=thickness, X=X)
    d = _pack([(p, 0, 0)], h, w, _lib.GRID_OUT_F32_CHW, 3, "rgb", 1.0, 0)
    out = np.zeros((h, w), np.float32)
    assert lib().hc_grid_alpha(ctypes.byref(d), _p(out), _p(out)) == 0
    return out


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def unit(w):
    """the largest float32 u with 150 u <= w, at most 17.7"""
    u = np.float32(w) / np.float32(150)
    if float(u) * 150.0 > w:
        u = np.nextafter(u, np.float32(0))
    return min(u, MAX_UNIT)


def baseline(u, h, bottom):
    return h - int(np.float32(5) * u) if bottom else int(np.float32(10) * u)


def py_format(x):
    """Python's own f"{x:.3f}" inside the stated domain; the clamped value outside it"""
    x = float(np.float32(x))
    if np.isfinite(x) and abs(x) >= 999999.9995:
        return ("-" if x < 0 else "") + "999999.999"
    return f"{x:.3f}"


def expand(label, value=None):
    """the characters a label draws: the slot filled as Python formats it, bytes outside 32..126 as '?'"""
    raw = label.encode("utf-8") if isinstance(label, str) else bytes(label)
    if value is not None:
        raw = raw.replace(SLOT, py_format(value).encode(), 1)
    return bytes(c if 32 <= c <= 126 else ord("?") for c in raw)


def line_bitmap(chars, font):
    """(7, 6 n) array of 0 / 1: a cell per character, its sixth column empty"""
    bm = np.zeros((7, 6 * len(chars)), np.float64)
    for i, c in enumerate(chars):
        for r in range(7):
            for col in range(5):
                bm[r, 6 * i + col] = (int(font[c - 32, r]) >> (4 - col)) & 1
    return bm


def coverage64(chars, w, h, font, bottom=False, bold=True, X=15):
    """Coverage (h, w): the sample coordinates in float32 exactly as the header forms them (every step is one IEEE operation),
    the bilinear sample itself in float64."""
    f32 = np.float32
    u = unit(w)
    base = baseline(u, h, bottom)
    top = f32(base) - f32(7) * u
    bm = line_bitmap(chars, font)
    padded = np.zeros((7 + 2, bm.shape[1] + 2))
    padded[1:-1, 1:-1] = bm

    def tex(gc, r):
        inside = (gc >= -1) & (gc <= bm.shape[1]) & (r >= -1) & (r <= 7)
        return np.where(inside, padded[np.clip(r + 1, 0, 8), np.clip(gc + 1, 0, bm.shape[1] + 1)], 0.0)

    ly = np.arange(h, dtype=np.float32)[:, None]
    lx = np.arange(w, dtype=np.float32)[None, :]
    fy = ((ly + f32(0.5) - top) / u - f32(0.5)).astype(np.float32)
    gx = ((lx + f32(0.5) - f32(X)) / u).astype(np.float32)

    def sample(fx):
        fx, fyb = np.broadcast_arrays(fx, fy)
        xf, yf = np.floor(fx), np.floor(fyb)
        tx, ty = (fx - xf).astype(np.float64), (fyb - yf).astype(np.float64)
        gc, r = xf.astype(np.int64), yf.astype(np.int64)
        a = (1 - ty) * ((1 - tx) * tex(gc, r) + tx * tex(gc + 1, r)) + ty * ((1 - tx) * tex(gc, r + 1) + tx * tex(gc + 1, r + 1))
        return np.where((fyb > -1) & (fyb < 7) & (fx > -1) & (len(chars) > 0), a, 0.0)

    fx = (gx - f32(0.5)).astype(np.float32)
    a = sample(fx)
    if bold:
        a = np.maximum(a, sample((fx - f32(0.5)).astype(np.float32)))
    return a


def blend64(x, a, colour):
    x = np.asarray(x, np.float64)
    return np.where(a > 0, (1 - a) * x + a * colour, x)


def torch_save_image_u8(x):
    """torchvision.utils.save_image's conversion (test.py:182-195) of a CPU tensor"""
    return x.clone().mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)


def numpy_clip_u8(x):
    """train.py:365"""
    with np.errstate(over="ignore"):
        return np.clip(np.asarray(x, np.float32) * 255, 0, 255).astype(np.uint8)
