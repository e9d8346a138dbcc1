"""The oracle of the training objective: a line-by-line torch restatement of the reference's
models/cage_net.py:214, 226 and train.py:190-244, the random batches of its tests, and the g++ build of csrc/objective_math.h.
float64 gives the tolerances their reference; float32 on the GPU is the timing baseline (tools/time_objective.py)."""
import ctypes
import os
import subprocess

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
KEYS = ("l1", "ssim", "sil_l1", "scale_energy", "fm_energy", "frame_encoding", "optimizable_poses", "blur_weights", "vgg")
KEY_ORDER = ("color_loss", "sil_loss", "scale_loss", "fme_loss", "blur_loss", "vgg_loss", "bg_loss", "codes_reg", "total_loss")
WEIGHTS = dict(lambda_dssim=0.2, rgb_weight=1.0, sil_weight=0.5, fme_weight=0.1, blur_weight=0.05, vgg_weight=0.02)
FWD_RTOL = 1e-5          # forward scalars against the float64 restatement of the same float32 inputs


def scale_energy(scaling, delta_scale=None, activation="exp", dtype=torch.float64):
    """cage_net.py:214 + :226 -> (1,)"""
    x = scaling.to(dtype) if delta_scale is None else scaling.to(dtype) + delta_scale.to(dtype)
    scales = torch.exp(x) if activation == "exp" else x                   # :214  scales = self.scaling_activation(self.scaling + delta_scale)
    return torch.mean(torch.mean(scales**2, axis=1))[None]               # :226


def objective(frames, weights, dtype=torch.float64):
    """train.py:190-244 over what :190-192 and the garment package hand it -> (total, losses dict in the reference's key order).
    Terms the reference leaves as the Python int 0 (absent entries, bg_loss) come back as 0-d zeros."""
    lambda_dssim, rgb_weight, sil_weight = weights["lambda_dssim"], weights["rgb_weight"], weights["sil_weight"]
    fme_weight, blur_weight, vgg_weight = weights["fme_weight"], weights["blur_weight"], weights["vgg_weight"]
    c = lambda t: None if t is None else t.to(dtype)
    perceptual_loss, color_loss, fme_loss, scale_loss, sil_loss, bg_loss, blur_loss, code_loss = [], [], [], [], [], [], [], []
    for frame in frames:
        rgb_l1, sil_l1, rgb_ssim = c(frame["l1"]), c(frame["sil_l1"]), c(frame["ssim"])
        blur_weights, optimizable_poses = c(frame.get("blur_weights")), c(frame.get("optimizable_poses"))
        color = (1.0 - lambda_dssim) * rgb_l1 + lambda_dssim * (1.0 - rgb_ssim)                        # :193
        blur_reg = (blur_weights - 1.0).abs().mean() if blur_weights is not None else -1               # :194
        code_reg = torch.mean(c(frame["frame_encoding"]) ** 2) * 0.001                                 # :195
        l2_poses = 0
        if optimizable_poses is not None:
            l2_poses = torch.mean(torch.mean(optimizable_poses**2, axis=-1)) * 0.0075                  # :198
        color_loss.append(color)
        sil_loss.append(sil_l1)
        code_loss.append(code_reg + l2_poses)
        scale_loss.append(c(frame["scale_energy"]) * 175.0)                                            # :203
        fm_energy = c(frame.get("fm_energy"))
        if fm_energy is not None:
            fme_loss.append(fm_energy.mean(dim=0) + 3.0)                                               # :207
        if not isinstance(blur_reg, int):
            blur_loss.append(blur_reg)
        if frame.get("vgg") is not None:
            perceptual_loss.append(c(frame["vgg"]))                                                    # :212-214
    color_loss = torch.stack(color_loss).mean() * rgb_weight                                           # :218
    sil_loss = torch.stack(sil_loss).mean() * sil_weight
    code_loss = torch.stack(code_loss).mean()
    scale_loss = torch.stack(scale_loss).mean()
    bg_loss = 0                                                                                        # :222 (the list stays empty)
    loss = 0
    loss += color_loss
    loss += sil_loss
    loss += bg_loss
    loss += code_loss
    loss += scale_loss
    fm = 0
    if len(fme_loss) > 0:
        fm = torch.stack(fme_loss).mean() * fme_weight
        loss += fm
    blur = 0
    if len(blur_loss) > 0:
        blur = torch.stack(blur_loss).mean() * blur_weight
        loss += blur
    vgg = 0
    if len(perceptual_loss) > 0:
        vgg = torch.stack(perceptual_loss).mean() * vgg_weight
        loss += vgg
    losses = {"color_loss": color_loss, "sil_loss": sil_loss, "scale_loss": scale_loss, "fme_loss": fm, "blur_loss": blur,
              "vgg_loss": vgg, "bg_loss": bg_loss, "codes_reg": code_loss, "total_loss": loss}
    zero = torch.zeros((), dtype=dtype, device=loss.device)
    return loss, {k: (v if torch.is_tensor(v) else zero) for k, v in losses.items()}


def make_frames(B, n_cages=1, D=32, poses=87, fm=True, blur=True, vgg=True, seed=0, device="cpu", requires_grad=False, as_views=False):
    """Random frames at the magnitudes of a training run (losses in [0,1], energies of a few 1e-4, fm_energy in (-3,3), codes
    of norm ~0.1, blur weights around 1).  as_views: every entry is a view of a larger tensor at an odd storage offset."""
    g = torch.Generator().manual_seed(1000 * seed + 17 * B + n_cages + D)
    frames = []
    for _ in range(B):
        fr = {"l1": 0.2 * torch.rand((), generator=g), "ssim": torch.rand((), generator=g), "sil_l1": 0.1 * torch.rand((), generator=g),
              "scale_energy": 1e-3 * torch.rand(n_cages, generator=g), "fm_energy": (6 * torch.rand(n_cages, generator=g) - 3) if fm else None,
              "frame_encoding": 0.1 * torch.randn(D, generator=g),
              "optimizable_poses": 0.5 * torch.randn(1, poses, generator=g) if poses else None,
              "blur_weights": (1 + 0.3 * torch.randn(1, 3, generator=g)) if blur else None, "vgg": 2 * torch.rand((), generator=g) if vgg else None}
        out = {}
        for k, v in fr.items():
            if v is None:
                out[k] = None
                continue
            if as_views:
                big = torch.zeros(v.numel() + 5)
                big[3:3 + v.numel()] = v.reshape(-1)
                big = big.to(device).requires_grad_(requires_grad)
                out[k] = big[3:3 + v.numel()].view(v.shape)
                out["_leaf_" + k] = big
            else:
                out[k] = v.to(device).requires_grad_(requires_grad)
        frames.append(out)
    return frames


def leaves(frames):
    """[(frame, key, leaf tensor)] of everything make_frames made differentiable"""
    out = []
    for f, fr in enumerate(frames):
        for k in KEYS:
            t = fr.get("_leaf_" + k, fr.get(k))
            if t is not None and t.requires_grad:
                out.append((f, k, t))
    return out


def grad_close(a, b):
    """the project's gradient rule, on every element: |a - b| <= 1e-3 |b| + 1e-6 max|b|"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return bool(((a - b).abs() <= 1e-3 * b.abs() + 1e-6 * b.abs().max()).all())


# ---- csrc/objective_math.h under g++ -------------------------------------------------------------------------------------------
class Entry(ctypes.Structure):
    _fields_ = [("ptr", ctypes.c_void_p), ("len", ctypes.c_int32), ("goff", ctypes.c_int32)]


class Desc(ctypes.Structure):
    _fields_ = [("n_frames", ctypes.c_int32), ("reserved", ctypes.c_int32)] + \
               [(n, ctypes.c_float) for n in ("lambda_dssim", "rgb_weight", "sil_weight", "fme_weight", "blur_weight", "vgg_weight")] + \
               [("entry", Entry * (16 * 9))]


def objcheck():
    src = os.path.join(ROOT, "tests", "hostcheck", "objcheck.cpp")
    out_dir = os.path.join(ROOT, "tests", "hostcheck", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libobjcheck.so")
    deps = [src, os.path.join(ROOT, "d3ga_amd", "csrc", "objective_math.h"), os.path.join(ROOT, "include", "d3ga.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", so])
    lib = ctypes.CDLL(so)
    lib.hc_scale_energy.restype = ctypes.c_float
    return lib


def host_desc(frames, weights, offsets=None):
    """(Desc, keep-alive arrays, total gradient floats) of CPU frames for the g++ build; offsets: True -> consecutive gradient slots"""
    d = Desc()
    d.n_frames = len(frames)
    for k, v in weights.items():
        setattr(d, k, v)
    keep, at = [], 0
    for f, fr in enumerate(frames):
        for slot, k in enumerate(KEYS):
            t = fr.get(k)
            if t is None:
                continue
            a = np.ascontiguousarray(t.detach().numpy().reshape(-1), np.float32)
            keep.append(a)
            e = d.entry[f * 9 + slot]
            e.ptr, e.len, e.goff = a.ctypes.data, a.size, (at if offsets else -1)
            at += a.size if offsets else 0
    return d, keep, at


def host_forward(lib, frames, weights, status=None):
    """hc_objective_fwd -> (terms float32 (9,), status int32 (16,))"""
    d, keep, _ = host_desc(frames, weights)
    terms = np.full(9, np.nan, np.float32)
    status = np.zeros(16, np.int32) if status is None else status
    assert lib.hc_objective_fwd(ctypes.byref(d), terms.ctypes.data_as(ctypes.c_void_p), status.ctypes.data_as(ctypes.c_void_p)) == 0
    return terms, status


def host_backward(lib, frames, weights, g=1.0):
    """hc_objective_bwd -> {(frame, key): gradient array}"""
    d, keep, n = host_desc(frames, weights, offsets=True)
    grads = np.full(n, np.nan, np.float32)
    assert lib.hc_objective_bwd(ctypes.byref(d), ctypes.c_float(g), grads.ctypes.data_as(ctypes.c_void_p)) == 0
    out = {}
    for f, fr in enumerate(frames):
        for slot, k in enumerate(KEYS):
            e = d.entry[f * 9 + slot]
            if e.ptr:
                out[(f, k)] = grads[e.goff:e.goff + e.len]
    return out
