"""The image tail (d3ga_amd/image_tail.py) against the same layer written with ATen on the GPU -- F.pad(reflect) + depth-wise
F.conv2d + the mixes, and the eight-line target composition of train.py:182-188 -- which is what a user without these
kernels runs.  Device events around every call, the two sides alternating call by call in one process: median / p10 / p90 in
microseconds, forward and forward + backward, at 1080x1920 and 747x1022.

    python tools/time_image_tail.py [--iters 200] [--warmup 30] [--out DIR]     -> DIR/image_tail_<H>x<W>.json (default profiles/)
    python tools/time_image_tail.py --trace-target 1080x1920                    the HIP side alone, 50 steps: the target of a
        `rocprofv3 --kernel-trace --stats -- python tools/time_image_tail.py --trace-target HxW` run of its own
    python tools/time_image_tail.py --kernel-stats FILE.csv --size HxW --out DIR  adds the per-kernel averages of such a run
        and their share of the HBM roofline (forward 8 C H W bytes, backward 12 C H W bytes, 8.0 TB/s) to the JSON
"""
import argparse
import csv
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_BYTES_PER_S = 8.0e12
SIZES = [(1080, 1920), (747, 1022)]
KERNELS = {"blur_mix_kernel<false>": ("forward", 8), "blur_mix_kernel<true>": ("backward", 12)}      # name -> (tag, bytes per element)


def taps(k, device):
    sigma = 0.15 * k + 0.35
    x = torch.linspace(-(k - 1) * 0.5, (k - 1) * 0.5, k, device=device)
    g = torch.exp(-0.5 * (x / sigma) ** 2)
    return g / g.sum()


def aten_blur(img, k2, k):
    C = img.shape[0]
    x = F.pad(img[None], [k // 2] * 4, mode="reflect")
    return F.conv2d(x, k2.expand(C, 1, k, k), groups=C)[0]


def aten_learnable_blur(img, weights_raw, cam, k3, k7):
    w = torch.softmax(weights_raw[cam], dim=-1)
    return w[0] * img + w[1] * aten_blur(img, k3, 3) + w[2] * aten_blur(img, k7, 7)


def aten_compose(image, alpha, silhouette, boundary_fg, bg):
    gt_alpha = alpha.expand(3, -1, -1)
    gt_silhouette = silhouette * gt_alpha
    gt_image = image * gt_alpha + (1 - gt_alpha) * bg[:, None, None]
    b = 1. - boundary_fg.float()
    gt_image = gt_image * b + (1. - b) * bg[:, None, None]
    return gt_image, gt_silhouette * b


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


def make(H, W):
    dev = "cuda"
    g = torch.Generator().manual_seed(H + W)
    t = lambda *s: torch.rand(*s, generator=g).to(dev)
    return dict(img=t(3, H, W).requires_grad_(True), wr=torch.randn(4, 3, generator=g).to(dev).requires_grad_(True),
                up=torch.randn(3, H, W, generator=g).to(dev), image=t(3, H, W), alpha=t(1, H, W), sil=t(3, H, W),
                bfg=t(1, H, W) > 0.8, bg=t(3), k3=torch.outer(taps(3, dev), taps(3, dev)), k7=torch.outer(taps(7, dev), taps(7, dev)))


def sides(d, cam=2):
    from d3ga_amd.image_tail import compose_target, learnable_blur

    def fb(fn):
        def run():
            d["img"].grad = d["wr"].grad = None
            fn().backward(d["up"])
        return run
    hip = lambda: learnable_blur(d["img"], d["wr"], cam)
    aten = lambda: aten_learnable_blur(d["img"], d["wr"], cam, d["k3"], d["k7"])

    def nograd(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run
    return {"fwd": {"hip": nograd(hip), "aten": nograd(aten)}, "fwd_bwd": {"hip": fb(hip), "aten": fb(aten)},
            "compose": {"hip": lambda: compose_target(d["image"], d["alpha"], d["sil"], d["bfg"], d["bg"]),
                        "aten": nograd(lambda: aten_compose(d["image"], d["alpha"], d["sil"], d["bfg"], d["bg"]))}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles"))
    ap.add_argument("--trace-target")
    ap.add_argument("--kernel-stats")
    ap.add_argument("--size")
    a = ap.parse_args()
    if a.kernel_stats:                                      # no GPU needed: fold a rocprofv3 kernel_stats.csv into the JSON
        H, W = (int(v) for v in a.size.split("x"))
        path = os.path.join(a.out, f"image_tail_{H}x{W}.json")
        rec = json.load(open(path)) if os.path.exists(path) else {"size": [H, W]}
        rec["kernels"] = {}
        for row in csv.DictReader(open(a.kernel_stats)):
            for key, (tag, per) in KERNELS.items():
                if key in row["Name"]:
                    us = float(row["AverageNs"]) / 1e3
                    floor = per * 3 * H * W / HBM_BYTES_PER_S * 1e6
                    rec["kernels"][tag] = {"name": row["Name"], "calls": int(row["Calls"]), "avg_us": round(us, 2),
                                           "algorithmic_bytes": per * 3 * H * W, "hbm_floor_us": round(floor, 2),
                                           "roofline_share": round(floor / us, 3)}
            if "blur_finish_kernel" in row["Name"] or "compose_target_kernel" in row["Name"]:
                rec["kernels"][row["Name"].split("(")[0].split("::")[-1]] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 2)}
        json.dump(rec, open(path, "w"), indent=1)
        print(json.dumps(rec["kernels"]))
        return
    assert torch.cuda.is_available(), "a timing needs the GPU"
    if a.trace_target:
        H, W = (int(v) for v in a.trace_target.split("x"))
        s = sides(make(H, W))
        for _ in range(50):
            s["fwd_bwd"]["hip"]()
            s["compose"]["hip"]()
        torch.cuda.synchronize()
        return
    os.makedirs(a.out, exist_ok=True)
    for (H, W) in SIZES:
        d = make(H, W)
        s = sides(d)
        with torch.no_grad():                               # faster and different is not faster
            err = float((s["fwd"]["hip"]() - s["fwd"]["aten"]()).abs().max())
        assert err <= 1e-4, err
        rec = {"size": [H, W], "iters": a.iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
               "max_abs_hip_vs_aten": err}
        for what, fns in s.items():
            us = alternate(fns, max(a.iters, 100), max(a.warmup, 20))
            rec[what] = {n: stats(v) for n, v in us.items()}
            rec[what]["speedup_median"] = round(rec[what]["aten"]["median_us"] / rec[what]["hip"]["median_us"], 2)
            # the condition: the HIP op is not slower than ATen beyond the spread of ATen's own repeats
            rec[what]["hip_not_slower"] = bool(rec[what]["hip"]["median_us"] <= rec[what]["aten"]["p90_us"])
            print(f"{H}x{W} {what}: hip {rec[what]['hip']} aten {rec[what]['aten']} x{rec[what]['speedup_median']}")
        path = os.path.join(a.out, f"image_tail_{H}x{W}.json")
        old = json.load(open(path)) if os.path.exists(path) else {}
        if "kernels" in old:
            rec["kernels"] = old["kernels"]
        json.dump(rec, open(path, "w"), indent=1)


if __name__ == "__main__":
    main()
