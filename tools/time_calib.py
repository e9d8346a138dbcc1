"""Colour calibration and pixel bias (d3ga_amd/calibration.py) against the ATen expressions they replace, on the GPU: the
reference's `rbg * w + b` with its `params.register_hook(... 1e-1)` (lib/calibration.py:39-56) and `image + F.interpolate(
bias[idxs], size=(H, W), mode='bilinear')` (models/color_calib.py:257, models/trainer.py:128-131).  Device events around every
call, the two sides alternating call by call in one process: median / p10 / p90 in microseconds, forward and forward +
backward, at 135k and 500k Gaussians and at 1022x747 with 160 cameras.

    python tools/time_calib.py [--iters 200] [--warmup 30] [--out DIR]     -> DIR/calib_<size>.json (default profiles/)

The events time the op as a user calls it (launches plus the Python layer's enqueue work).  `kernel_only` times the HIP op
again inside a captured graph of 20 calls, one twentieth of a replay: the kernels without the host, which is what the share
of the HBM roofline is formed from (algorithmic bytes per Gaussian and view: forward 24, backward 36, backward without
dL/drgb 24; per pixel: fused bias forward 8 C, bias backward 4 C)."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_BYTES_PER_S = 8.0e12
N_CAMERAS = 160
GAUSSIANS = [135_000, 500_000]
IMAGE = (1022, 747)


def alternate(fns, iters, warmup):
    """fns: name -> callable; every round runs each once, timed by its own pair of events -> name -> us per call (array)"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ev = {n: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)] for n in fns}
    for i in range(iters):
        for n, fn in fns.items():
            a, b = ev[n][i]
            a.record()
            fn()
            b.record()
    torch.cuda.synchronize()
    return {n: np.array([a.elapsed_time(b) * 1e3 for a, b in ev[n]]) for n in fns}


def stats(us):
    return {"median_us": round(float(np.median(us)), 2), "p10_us": round(float(np.percentile(us, 10)), 2),
            "p90_us": round(float(np.percentile(us, 90)), 2)}


def graph_time(fn, calls=20, reps=30):
    """us per call of `fn` inside a captured graph of `calls` calls (median over `reps` replays)"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    us = alternate({"g": g.replay}, reps, 3)["g"]
    return float(np.median(us)) / calls


def nograd(fn):
    def run():
        with torch.no_grad():
            return fn()
    return run


def fwd_bwd(fn, leaves, up):
    def run():
        for t in leaves:
            t.grad = None
        fn().backward(up)
    return run


def colour_sides(P):
    from d3ga_amd.calibration import color_calib
    g = torch.Generator().manual_seed(P)
    rgb = torch.rand(P, 3, generator=g).cuda().requires_grad_(True)
    cor = torch.cat([1 + 0.1 * torch.randn(N_CAMERAS, 3, generator=g), 0.1 * torch.randn(N_CAMERAS, 3, generator=g)], 1).cuda().requires_grad_(True)
    up = torch.randn(P, 3, generator=g).cuda()
    cam = 7

    def aten():
        params = cor[cam]
        w, b = params[:3], params[3:]
        out = rgb * w + b
        if params.requires_grad and torch.is_grad_enabled():
            params.register_hook(lambda gr: gr * 1e-1)
        return out
    hip = lambda: color_calib(rgb, cor, cam, 0, grad_scale=0.1)
    with torch.no_grad():
        assert torch.equal(hip(), aten())
    rgb_c = rgb.detach()
    hip_c = lambda: color_calib(rgb_c, cor, cam, 0, grad_scale=0.1)
    return {"fwd": {"hip": nograd(hip), "aten": nograd(aten)},
            "fwd_bwd": {"hip": fwd_bwd(hip, (rgb, cor), up), "aten": fwd_bwd(aten, (rgb, cor), up)}}, \
           {"fwd": (nograd(hip), 24 * P), "fwd_bwd": (fwd_bwd(hip, (rgb, cor), up), 60 * P),
            "fwd_bwd_no_drgb": (fwd_bwd(hip_c, (cor,), up), 48 * P)}


def bias_sides(H, W):
    from d3ga_amd.calibration import pixel_bias_add
    g = torch.Generator().manual_seed(H)
    bias = (0.05 * torch.randn(N_CAMERAS, 1, W // 8, H // 8, generator=g)).cuda().requires_grad_(True)
    img = torch.rand(3, H, W, generator=g).cuda().requires_grad_(True)
    up = torch.randn(3, H, W, generator=g).cuda()
    cam = 7
    idx = torch.tensor([cam], device="cuda")
    aten = lambda: img + F.interpolate(bias[idx], size=(H, W), mode="bilinear")[0]
    hip = lambda: pixel_bias_add(img, bias, cam)
    with torch.no_grad():
        err = float((hip() - aten()).abs().max())
    assert err <= 1e-5, err
    return {"fwd": {"hip": nograd(hip), "aten": nograd(aten)},
            "fwd_bwd": {"hip": fwd_bwd(hip, (img, bias), up), "aten": fwd_bwd(aten, (img, bias), up)}}, \
           {"fwd": (nograd(hip), 24 * H * W), "fwd_bwd": (fwd_bwd(hip, (img, bias), up), 36 * H * W + 4 * bias.numel())}


def record(name, sides, kernels, a, extra):
    rec = dict(extra, iters=a.iters, warmup=a.warmup, device=torch.cuda.get_device_name(0), n_cameras=N_CAMERAS)
    for what, fns in sides.items():
        us = alternate(fns, max(a.iters, 100), max(a.warmup, 20))
        rec[what] = {n: stats(v) for n, v in us.items()}
        rec[what]["speedup_median"] = round(rec[what]["aten"]["median_us"] / rec[what]["hip"]["median_us"], 2)
        print(f"{name} {what}: hip {rec[what]['hip']} aten {rec[what]['aten']} x{rec[what]['speedup_median']}")
    rec["kernel_only"] = {}
    for what, (fn, nbytes) in kernels.items():
        us = graph_time(fn)
        floor = nbytes / HBM_BYTES_PER_S * 1e6
        rec["kernel_only"][what] = {"us": round(us, 2), "algorithmic_bytes": nbytes, "hbm_floor_us": round(floor, 2),
                                    "roofline_share": round(floor / us, 3)}
        print(f"{name} kernel_only {what}: {rec['kernel_only'][what]}")
    json.dump(rec, open(os.path.join(a.out, f"calib_{name}.json"), "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    os.makedirs(a.out, exist_ok=True)
    for P in GAUSSIANS:
        sides, kernels = colour_sides(P)
        record(f"{P // 1000}k", sides, kernels, a, {"gaussians": P})
    H, W = IMAGE
    sides, kernels = bias_sides(H, W)
    record(f"{H}x{W}", sides, kernels, a, {"size": [H, W], "bias_map": [W // 8, H // 8]})


if __name__ == "__main__":
    main()
