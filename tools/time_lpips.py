"""LPIPS (d3ga_amd/lpips.py) against the same chain written with F.conv2d / F.max_pool2d on the same GPU with the same weights
(true VGG16 widths, seeded He weights and heads: the timing does not depend on the values): the metric of one image pair at
full resolution, as recorder/heatmap.py:40 asks for it.  Sizes: 747 x 1022 (the Goliath frames) and 1080 x 1920.  Also what
batching the pair bought: the module (fake and target as ONE batch of two per layer) against the same launches run as two
chains of one image each, same library.  Device events around every call, the sides alternating call by call in one process:
median / p10 / p90 in microseconds of --iters calls after --warmup.

    python tools/time_lpips.py [--iters 50] [--warmup 10] [--out DIR]      -> DIR/lpips_<H>x<W>.json (default profiles/)

A pass of the chain over one image is `macs` multiply-adds (two images per call); the HIP path spends six bf16 MFMA products
per multiply-add (f32-equivalent arithmetic).  No speed bar is set: the ratio is reported whichever way it falls.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SIZES = ((747, 1022), (1080, 1920))
KEYS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
WIDTHS = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
POOL_BEFORE = (2, 4, 7, 10)
TAPS = (1, 3, 6, 9, 12)
SHIFT, SCALE = (-.030, -.088, -.188), (.458, .448, .450)


def make_weights(dev):
    g = torch.Generator().manual_seed(5)
    sd, cin = {}, 3
    for k, c in zip(KEYS, WIDTHS):
        sd[f"features.{k}.weight"] = (torch.randn(c, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5).to(dev)
        sd[f"features.{k}.bias"] = ((torch.rand(c, generator=g) - 0.5) * 0.2).to(dev)
        cin = c
    for t, i in enumerate(TAPS):
        sd[f"lin{t}.model.1.weight"] = (torch.rand(1, WIDTHS[i], 1, 1, generator=g) * 0.2).to(dev)
    return sd


def torch_lpips(sd, fake, target):
    shift = torch.tensor(SHIFT, device=fake.device).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, device=fake.device).view(1, 3, 1, 1)
    x = (torch.stack([fake, target]) - shift) / scale
    value, tap = 0, 0
    for i, k in enumerate(KEYS):
        if i in POOL_BEFORE:
            x = F.max_pool2d(x, 2)
        x = F.relu(F.conv2d(x, sd[f"features.{k}.weight"], sd[f"features.{k}.bias"], padding=1))
        if i in TAPS:
            n = x / (x.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10)
            value = value + ((n[0] - n[1]) ** 2 * sd[f"lin{tap}.model.1.weight"][0]).sum(dim=0).mean()
            tap += 1
    return value


def hip_two_chains(mod, fake, target, bufs):
    """The module's launches with the pair NOT batched: each layer runs once per image (N = 1), then the same distance."""
    from d3ga_amd import lpips as L
    from d3ga_amd.perceptual import conv3x3_n, maxpool2_n
    _, _, H, W = fake.shape
    pl = L.plan(H, W)
    value = bufs["value"]
    cur = [L.scale_input(img, mod.normalize, out=bufs["pp"][s][0][:H * W * 3].view(1, H, W, 3)) for s, img in enumerate((fake, target))]
    side, cin, tap = 1, 3, 0
    for i, c in enumerate(mod.widths):
        h, w = pl.convs[i]
        if i in POOL_BEFORE:
            cur = [maxpool2_n(cur[s], out=bufs["pp"][s][side][:h * w * cin].view(1, h, w, cin)) for s in range(2)]
            side ^= 1
        cur = [conv3x3_n(cur[s], mod._panels[i], mod._biases[i], c, out=bufs["pp"][s][side][:h * w * c].view(1, h, w, c)) for s in range(2)]
        side ^= 1
        if i in TAPS:
            L.tap_distance(cur[0], cur[1], mod._lins[tap], False, value, tap > 0, bufs["partials"])
            tap += 1
        cin = c
    return value


def macs(H, W):
    h, w, cin, n = H, W, 3, 0
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
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    from d3ga_amd import _lib
    from d3ga_amd import lpips as L
    dev = torch.device("cuda", 0)
    sd = make_weights(dev)
    mod = L.LPIPS("vgg", sd).to(dev).prepare()
    os.makedirs(a.out, exist_ok=True)
    for H, W in SIZES:
        g = torch.Generator().manual_seed(H)
        target = torch.rand(3, H, W, generator=g).to(dev)
        fake = (target + 0.1 * torch.randn(3, H, W, generator=g).to(dev)).clamp(0, 1)
        mod.prepare(H, W, 1)
        total, one, part = L.scratch_bytes(1, H, W, WIDTHS)
        half = one // 8                                         # floats of one image's share of a ping-pong buffer
        bufs = {"pp": [[torch.empty(half, device=dev), torch.empty(half, device=dev)] for _ in range(2)],
                "partials": torch.empty(_lib.LPIPS_PARTIALS, device=dev), "value": torch.empty(1, device=dev)}
        f4, t4 = fake[None].contiguous(), target[None].contiguous()
        with torch.no_grad():
            fns = {"torch": lambda: torch_lpips(sd, fake, target), "hip": lambda: mod(fake, target),
                   "hip_two_chains": lambda: hip_two_chains(mod, f4, t4, bufs)}
            vh, vt, v2 = float(fns["hip"]()), float(fns["torch"]()), float(fns["hip_two_chains"]())
            us = alternate(fns, a.iters, a.warmup)
        r = {k: stats(v) for k, v in us.items()}
        rec = {"H": H, "W": W, "iters": a.iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "macs_per_image": macs(H, W),
               "work_area_bytes": total, "value_hip": vh, "value_torch": vt, "value_hip_two_chains": v2, "two_chains_bit_identical": vh == v2, **r,
               "torch_over_hip_median": round(r["torch"]["median_us"] / r["hip"]["median_us"], 3),
               "two_chains_over_batched_median": round(r["hip_two_chains"]["median_us"] / r["hip"]["median_us"], 3),
               "hip_f32_equivalent_tflops": round(2 * 2 * macs(H, W) / (r["hip"]["median_us"] * 1e-6) / 1e12, 1)}
        print(f"{H}x{W}: hip {r['hip']} two chains {r['hip_two_chains']} torch {r['torch']} torch/hip {rec['torch_over_hip_median']} "
              f"two/batched {rec['two_chains_over_batched_median']}")
        json.dump(rec, open(os.path.join(a.out, f"lpips_{H}x{W}.json"), "w"), indent=1)
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
