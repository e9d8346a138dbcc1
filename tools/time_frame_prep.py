"""Frame preparation (d3ga_amd/frame_prep.py) against a torch restatement of the reference sequence it replaces
(lib/batch.py:150-163, 180, 205-208, 236 with kornia's median_blur / dilation / erosion), on the GPU, at the Goliath frame
(747 x 1022) and at 1080 x 1920, B = 1.

    python tools/time_frame_prep.py [--iters 200] [--warmup 30] [--bench-steps 60] [--out DIR]
        -> DIR/frame_prep_<W>x<H>.json (default profiles/)

The torch side is written here from kornia's documented construction, not copied: the median as a one-hot 49-channel conv2d
followed by median(dim=2), dilation / erosion (engine="convolution") as a one-hot conv2d of the padded mask followed by a
maximum / minimum over the channel axis, then the reference's element-wise lines and its four boolean scatters.  Both sides
are timed with device events, alternating call by call in one process (median / p10 / p90 in microseconds), for the two
shipped flag sets: `goliath` (use_gamma_space) and `full` (use_gamma_space, erode_mask, use_close_holes).  `kernel_only` times
the HIP op inside a captured graph of 20 calls -- the kernel without the host -- and forms its share of the HBM roofline
from the 15 float planes per pixel that the algorithm has to move (image 3, seg_part 1, seg_fg 1 in; image 3, orig 3,
alpha 1, silhouette 3 out): 60 bytes per pixel, 51 with a uint8 image.  `step_ms` is the benchmark's training step of this
checkout (bench.py in a child process), for scale: frame preparation is not part of it, so it equals the parent commit's."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8.0e12
SIZES = [(747, 1022), (1080, 1920)]                          # (W, H)
CAGES = {"body": {"label_id": [1]}, "upper": {"label_id": [27]}, "lower": {"label_id": [16]}}
FLAG_SETS = {"goliath": dict(gamma=True, erode_mask=False, close_holes=False),
             "full": dict(gamma=True, erode_mask=True, close_holes=True)}


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
    return {"median_us": round(float(np.median(us)), 2), "p10_us": round(float(np.percentile(us, 10)), 2),
            "p90_us": round(float(np.percentile(us, 90)), 2)}


def graph_time(fn, calls=20, reps=30):
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
    return float(np.median(alternate({"g": g.replay}, reps, 3)["g"])) / calls


def one_hot_windows(x, k, fill):
    """(B,1,H,W) -> (B,k*k,H,W): channel j holds the j-th pixel of the k x k window, `fill` outside the image"""
    kernel = torch.eye(k * k, device=x.device).view(k * k, 1, k, k)
    return F.conv2d(F.pad(x, (k // 2,) * 4, value=fill), kernel)


def torch_sequence(image, seg_part, seg_fg, gamma, erode_mask, close_holes, white=True):
    """The reference's lines for B frames -> (image, orig_image, alpha, silhouette)"""
    seg_part = seg_part.int()
    fg = ((seg_part > 0) | (seg_fg > 0)).float()
    alpha = one_hot_windows(fg, 7, 0.0)[:, None].median(dim=2)[0]
    pairs = ([(7, 5)] if erode_mask else []) + ([(5, 5)] if close_holes else [])
    for kd, ke in pairs:
        alpha = one_hot_windows(alpha, kd, -1e4).amax(dim=1, keepdim=True)
        alpha = one_hot_windows(alpha, ke, 1e4).amin(dim=1, keepdim=True)
    frames = []
    for i in range(image.shape[0]):
        x = image[i] / 255.0
        if gamma:
            scale = torch.tensor([1.4, 1.1, 1.6], device=x.device).view(3, 1, 1)
            black = 3.0 / 255.0
            x = x * scale / 1.1
            x = torch.clamp(((1.0 / (1 - black)) * 0.95 * torch.clamp(x - black, 0, 2)).pow(0.5) - 15.0 / 255.0, 0, 2)
        img = x * fg[i] + (1.0 - fg[i]) if white else x * fg[i]
        s = seg_part[i]
        sil = torch.ones((s.shape[1], s.shape[2], 3), device=x.device) * float(white)
        masks = []
        for name in ("upper", "lower", "face"):
            m = torch.zeros_like(s).bool()
            for label in (CAGES[name]["label_id"] if name in CAGES else [-1]):
                if label != -1:
                    m = m | (s == label)
            masks.append(m)
        body = ~(s == 0) & ~masks[0] & ~masks[1] & ~masks[2]
        for m, rgb in zip(masks + [body], ((1.0, 0, 0), (0, 1.0, 0), (0.5, 0.5, 0.5), (0, 0, 1.0))):
            sil[m[0]] = torch.tensor(rgb, device=x.device)
        frames.append((img, x, alpha[i], sil.permute(2, 0, 1).float()))
    return [torch.stack(t) for t in zip(*frames)]


def synthetic_frame(W, H, seed):
    """A person-sized blob of labels with a ragged outline and a few holes, an image of integers 0..255"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
    body = ((xx / 0.45) ** 2 + (yy / 0.85) ** 2) < 1.0 + 0.05 * torch.randn(H, W, generator=g)
    seg = torch.where(body, torch.where(yy < -0.1, 27, torch.where(yy < 0.5, 16, 1)), 0).int()
    seg[torch.rand(H, W, generator=g) < 0.01] = 0
    seg_fg = (body & (torch.rand(H, W, generator=g) < 0.9)).float()
    image = torch.randint(0, 256, (1, 3, H, W), generator=g).float()
    return image.cuda(), seg[None, None].cuda().contiguous(), seg_fg[None, None].cuda().contiguous()


def bench_step_ms(steps):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "10"],
                         capture_output=True, text=True, check=True, cwd=ROOT).stdout
    line = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    for key in ("step_ms", "ms_per_step", "step_time_ms"):
        if key in line:
            return float(line[key]), line
    return None, line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--bench-steps", type=int, default=60, help="0: do not run bench.py for the step time")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    from d3ga_amd.frame_prep import FramePrep
    os.makedirs(a.out, exist_ok=True)
    step_ms, bench_line = (None, None)
    if a.bench_steps > 0:
        step_ms, bench_line = bench_step_ms(a.bench_steps)   # a child of its own, before this process opens the GPU
    for W, H in SIZES:
        image, seg, seg_fg = synthetic_frame(W, H, W)
        rec = {"size": [W, H], "B": 1, "iters": a.iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
               "step_ms": step_ms, "bench_line": bench_line}
        for name, fl in FLAG_SETS.items():
            prep = FramePrep({"train": {"use_gamma_space": fl["gamma"], "erode_mask": fl["erode_mask"],
                                        "use_close_holes": fl["close_holes"]}, "cages": CAGES})
            out = {n: torch.empty(1, c, H, W, device="cuda") for n, c in (("image", 3), ("orig_image", 3), ("alpha", 1), ("silhouette", 3))}
            hip = lambda: prep(image, seg, seg_fg, out=out)
            image8 = image.to(torch.uint8)
            hip8 = lambda: prep(image8, seg, seg_fg, out=out)
            ref = lambda: torch_sequence(image, seg, seg_fg, **fl)
            with torch.no_grad():
                got, want = hip(), ref()
                torch.cuda.synchronize()
                agree = {"alpha_equal": bool(torch.equal(got["alpha"], want[2])), "silhouette_equal": bool(torch.equal(got["silhouette"], want[3])),
                         "image_max_abs": float((got["image"] - want[0]).abs().max()), "orig_max_abs": float((got["orig_image"] - want[1]).abs().max())}
                assert agree["alpha_equal"] and agree["silhouette_equal"] and agree["image_max_abs"] <= 1e-5 and agree["orig_max_abs"] <= 1e-5, agree
                us = alternate({"hip": hip, "hip_u8": hip8, "torch": ref}, max(a.iters, 100), max(a.warmup, 20))
            r = {n: stats(v) for n, v in us.items()}
            r["speedup_median"] = round(r["torch"]["median_us"] / r["hip"]["median_us"], 2)
            r["agreement"] = agree
            r["kernel_only"] = {}
            for what, fn, nbytes in (("f32", hip, 60 * W * H), ("u8", hip8, 51 * W * H)):
                k_us = graph_time(fn)
                floor = nbytes / HBM_BYTES_PER_S * 1e6
                r["kernel_only"][what] = {"us": round(k_us, 2), "algorithmic_bytes": nbytes, "hbm_floor_us": round(floor, 2),
                                          "roofline_share": round(floor / k_us, 3), "achieved_TBps": round(nbytes / k_us * 1e-6, 3)}
            if step_ms:
                r["share_of_step"] = {"hip": round(r["hip"]["median_us"] / (step_ms * 1e3), 3), "torch": round(r["torch"]["median_us"] / (step_ms * 1e3), 3)}
            rec[name] = r
            print(f"{W}x{H} {name}: {json.dumps(r)}")
        json.dump(rec, open(os.path.join(a.out, f"frame_prep_{W}x{H}.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
