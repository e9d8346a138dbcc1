"""Float64 side of tests/test_gpu_field_glue.py: the element-wise ops around the field networks (csrc/encoding.hip) restated in
plain torch -- the output heads and the view directions -- with their derivatives in closed form, and the table of arguments
that d3ga_field_heads_* / d3ga_color_rows_* / d3ga_sh4_encoding_* refuse.  No project import: the library and its status codes
are handed in.  The SH encoding itself stays oracle.mlp.sh4_direction_encoding."""
import ctypes
import re

import torch

ACT = {"none": 0, "tanh": 1, "sigmoid": 2}          # act[h] of d3ga_field_heads_* (include/d3ga.h)


def heads(pred, spec):
    """pred (P,N), spec = ((width, "none" | "tanh" | "sigmoid", param), ...) with widths summing to N -> the list of (P, w_h)
    blocks: x, param * tanh(x), sigmoid(x + param)."""
    out, c = [], 0
    for w, act, param in spec:
        x = pred[:, c:c + w]
        out.append(x if act == "none" else param * torch.tanh(x) if act == "tanh" else torch.sigmoid(x + param))
        c += w
    if c != pred.shape[1]:
        raise ValueError(f"heads: widths sum to {c}, pred has {pred.shape[1]} columns")
    return out


def heads_slope(pred, spec):
    """d head / d pred, element by element (P,N): 1, param (1 - tanh^2 x), s (1 - s) with s = sigmoid(x + param)."""
    cols, c = [], 0
    for w, act, param in spec:
        x = pred[:, c:c + w]
        if act == "none":
            cols.append(torch.ones_like(x))
        elif act == "tanh":
            cols.append(param * (1.0 - torch.tanh(x) ** 2))
        else:
            s = torch.sigmoid(x + param)
            cols.append(s * (1.0 - s))
        c += w
    return torch.cat(cols, dim=1)


def view_dirs(means, campos):
    """(means - campos) / |means - campos|, row by row (models/cage_net.py:233-235)."""
    d = means - campos
    return d / torch.linalg.norm(d, dim=-1, keepdim=True)


def view_dirs_vjp(means, campos, g):
    """g^T d v / d means = (g - v (v . g)) / |means - campos|: the Jacobian (I - v v^T) / r is symmetric."""
    d = means - campos
    r = torch.linalg.norm(d, dim=-1, keepdim=True)
    v = d / r
    return (g - v * (v * g).sum(-1, keepdim=True)) / r


def status_codes(header_text):
    """{"OK": 0, "E_NULL": -1, ...} from the #define D3GA_OK / D3GA_E_* lines of include/d3ga.h."""
    return {k: int(v) for k, v in re.findall(r"#define\s+D3GA_(OK|E_[A-Z]+)\s+\(?(-?\d+)\)?", header_text)}


def _spec_arrays(width, act, param):
    return (None if width is None else (ctypes.c_int32 * len(width))(*width), None if act is None else (ctypes.c_int32 * len(act))(*act),
            None if param is None else (ctypes.c_float * len(param))(*param))


def check_heads_refusals(L, codes, pred, out, g, d_pred):
    """Every argument set d3ga_field_heads_fwd / _bwd refuse, one fault at a time, on library L: asserts the documented status.
    pred, out, g, d_pred: addresses (int) of buffers for (8, 6) floats -- any made-up non-NULL value where no device is present,
    as nothing is launched."""
    base = dict(P=8, N=6, n_heads=2, width=(4, 2), act=(1, 2), param=(0.5, 0.1))
    cases = [("n_heads 0", dict(n_heads=0), "E_CONFIG"), ("n_heads 5", dict(n_heads=5, width=(1, 1, 1, 1, 2), act=(0,) * 5, param=(0.0,) * 5), "E_CONFIG"),
             ("a width of 0", dict(width=(6, 0)), "E_CONFIG"), ("a negative width", dict(width=(7, -1)), "E_CONFIG"),
             ("act -1", dict(act=(-1, 2)), "E_CONFIG"), ("act 3", dict(act=(1, 3)), "E_CONFIG"),
             ("tanh with param 0", dict(param=(0.0, 0.1)), "E_CONFIG"), ("tanh with param -0", dict(param=(-0.0, 0.1)), "E_CONFIG"),
             ("NULL width", dict(width=None), "E_CONFIG"), ("NULL act", dict(act=None), "E_CONFIG"), ("NULL param", dict(param=None), "E_CONFIG"),
             ("widths short of N", dict(width=(3, 2)), "E_SIZE"), ("widths past N", dict(width=(4, 3)), "E_SIZE"),
             ("P < 0", dict(P=-1), "E_SIZE"), ("N == 0", dict(N=0), "E_SIZE"), ("N < 0", dict(N=-6), "E_SIZE")]
    vp = ctypes.c_void_p
    for what, change, want in cases:
        a = dict(base, **change)
        arrays = _spec_arrays(a["width"], a["act"], a["param"])
        assert L.d3ga_field_heads_fwd(a["P"], a["N"], a["n_heads"], *arrays, vp(pred), vp(out), None) == codes[want], ("fwd", what)
        assert L.d3ga_field_heads_bwd(a["P"], a["N"], a["n_heads"], *arrays, vp(out), vp(g), vp(g), None, None, vp(d_pred), None) == codes[want], ("bwd", what)
    arrays = _spec_arrays(base["width"], base["act"], base["param"])
    sizes = (base["P"], base["N"], base["n_heads"])
    assert L.d3ga_field_heads_fwd(*sizes, *arrays, None, vp(out), None) == codes["E_NULL"]
    assert L.d3ga_field_heads_fwd(*sizes, *arrays, vp(pred), None, None) == codes["E_NULL"]
    assert L.d3ga_field_heads_bwd(*sizes, *arrays, None, vp(g), vp(g), None, None, vp(d_pred), None) == codes["E_NULL"]
    assert L.d3ga_field_heads_bwd(*sizes, *arrays, vp(out), vp(g), vp(g), None, None, None, None) == codes["E_NULL"]


def check_encoding_refusals(L, codes, dirs, feats, x, enc, d_dirs, d_feats):
    """d3ga_color_rows_* with a feature count that is no multiple of 4 and with x / feats / d_x / d_feats 4 bytes off their
    16-byte alignment, d3ga_sh4_encoding_* with enc / d_enc 4 bytes off.  Addresses (int, 16-byte aligned) of buffers for 8
    rows: dirs (8,3), feats (8,8) + 1, x (8,24) + 1, enc (8,16) + 1, d_dirs (8,3), d_feats (8,8) + 1 floats."""
    vp = ctypes.c_void_p
    assert all(p % 16 == 0 for p in (feats, x, enc, d_feats))
    assert L.d3ga_color_rows_fwd(8, 6, vp(dirs), vp(feats), vp(x), None) == codes["E_SIZE"]
    assert L.d3ga_color_rows_bwd(8, 6, vp(dirs), vp(x), vp(d_dirs), vp(d_feats), None) == codes["E_SIZE"]
    assert L.d3ga_color_rows_fwd(8, 8, vp(dirs), vp(feats), vp(x + 4), None) == codes["E_CONFIG"]
    assert L.d3ga_color_rows_fwd(8, 8, vp(dirs), vp(feats + 4), vp(x), None) == codes["E_CONFIG"]
    assert L.d3ga_color_rows_bwd(8, 8, vp(dirs), vp(x + 4), vp(d_dirs), vp(d_feats), None) == codes["E_CONFIG"]
    assert L.d3ga_color_rows_bwd(8, 8, vp(dirs), vp(x), vp(d_dirs), vp(d_feats + 4), None) == codes["E_CONFIG"]
    assert L.d3ga_sh4_encoding_fwd(8, vp(dirs), vp(enc + 4), None) == codes["E_CONFIG"]
    assert L.d3ga_sh4_encoding_bwd(8, vp(dirs), vp(enc + 4), vp(d_dirs), None) == codes["E_CONFIG"]
