"""VGGLoss (d3ga_amd/perceptual.py) against the same chain written with F.conv2d / F.max_pool2d under autograd, on the same
GPU with the same weights (VGG19 widths, seeded He weights: the timing does not depend on the values): the loss of one image
pair, forward + backward into the predicted image, and the forward alone.  Sizes: 373 x 511 (ActorsHQ at half resolution)
and 747 x 1022 (the Goliath frames).  Device events around every call, the two sides alternating call by call in one
process: median / p10 / p90 in microseconds of --iters calls after --warmup.

    python tools/time_perceptual.py [--iters 100] [--warmup 20] [--out DIR]      -> DIR/perceptual_<H>x<W>.json (default profiles/)

A forward of the chain is `macs` multiply-adds per image (two images per step, and one more pass of about the same size for
the input gradient); the HIP path spends six bf16 MFMA products per multiply-add (f32-equivalent arithmetic).
`grad_max_abs_diff_over_max` in the record is a sanity figure, not a test: at these sizes a few of the millions of ReLU, pool
and sign decisions fall differently in two float32 evaluations, and each flip moves the gradient by a visible step
(tests/test_gpu_perceptual.py compares gradients at qualified seeds instead).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SIZES = ((373, 511), (747, 1022))
KEYS = (0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28)
WIDTHS = (64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512, 512)
POOL_BEFORE = (2, 4, 8, 12)
TAPS = (0, 2, 4, 8, 12)


def make_weights(dev):
    g = torch.Generator().manual_seed(5)
    sd, cin = {}, 3
    for k, c in zip(KEYS, WIDTHS):
        sd[f"features.{k}.weight"] = (torch.randn(c, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5).to(dev)
        sd[f"features.{k}.bias"] = ((torch.rand(c, generator=g) - 0.5) * 0.2).to(dev)
        cin = c
    return sd


def torch_loss(sd, pred, gt):
    s = F.interpolate(pred[None], scale_factor=0.5, mode="bilinear")
    with torch.no_grad():
        t = F.interpolate(gt[None], scale_factor=0.5, mode="bilinear")
    loss = 0
    for i, k in enumerate(KEYS):
        w, b = sd[f"features.{k}.weight"], sd[f"features.{k}.bias"]
        if i in POOL_BEFORE:
            s = F.max_pool2d(s, 2)
            with torch.no_grad():
                t = F.max_pool2d(t, 2)
        s = F.relu(F.conv2d(s, w, b, padding=1))
        with torch.no_grad():
            t = F.relu(F.conv2d(t, w, b, padding=1))
        if i in TAPS:
            loss = loss + (s - t).abs().mean()
    return loss


def macs(H, W):
    h, w, cin, n = H // 2, W // 2, 3, 0
    for i, c in enumerate(WIDTHS):
        if i in POOL_BEFORE:
            h, w = h // 2, w // 2
        n += h * w * 9 * cin * c
        cin = c
    return n


def alternate(fns, iters, warmup):
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
    return {"median_us": round(float(np.median(us)), 1), "p10_us": round(float(np.percentile(us, 10)), 1),
            "p90_us": round(float(np.percentile(us, 90)), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    from d3ga_amd.perceptual import VGGLoss
    dev = torch.device("cuda", 0)
    sd = make_weights(dev)
    mod = VGGLoss(5, sd).to(dev).prepare()
    os.makedirs(a.out, exist_ok=True)
    for H, W in SIZES:
        g = torch.Generator().manual_seed(H)
        gt = torch.rand(3, H, W, generator=g).to(dev)
        pred = (gt + 0.1 * torch.randn(3, H, W, generator=g).to(dev)).clamp(0, 1).requires_grad_(True)

        def hip_fb():
            (gr,) = torch.autograd.grad(mod(pred, gt), pred)
            return gr

        def torch_fb():
            (gr,) = torch.autograd.grad(torch_loss(sd, pred, gt), pred)
            return gr

        def hip_f():
            with torch.no_grad():
                return mod(pred, gt)

        def torch_f():
            with torch.no_grad():
                return torch_loss(sd, pred, gt)

        lh, lt = float(hip_f()), float(torch_f())
        gh, gtt = hip_fb(), torch_fb()
        rec = {"H": H, "W": W, "iters": a.iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "macs_per_forward": macs(H, W),
               "loss_hip": lh, "loss_torch": lt, "grad_max_abs_diff_over_max": float((gh - gtt).abs().max() / gtt.abs().max())}
        for name, fns in (("forward_backward", {"torch": torch_fb, "hip": hip_fb}), ("forward", {"torch": torch_f, "hip": hip_f})):
            us = alternate(fns, a.iters, a.warmup)
            r = {k: stats(v) for k, v in us.items()}
            r["torch_over_hip_median"] = round(r["torch"]["median_us"] / r["hip"]["median_us"], 3)
            passes = 3 if name == "forward_backward" else 2
            r["hip_f32_equivalent_tflops"] = round(2 * passes * macs(H, W) / (r["hip"]["median_us"] * 1e-6) / 1e12, 1)
            rec[name] = r
            print(f"{H}x{W} {name}: hip {r['hip']} torch {r['torch']} torch/hip {r['torch_over_hip_median']}")
        json.dump(rec, open(os.path.join(a.out, f"perceptual_{H}x{W}.json"), "w"), indent=1)
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
