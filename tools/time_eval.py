"""The evaluation tail (d3ga_amd/evaluation.py: Evaluator.add) against the reference's own per-frame sequence on the same
device tensors, at the Goliath frame (747 x 1022) and at 1080 x 1920, one frame per call.

    python tools/time_eval.py [--iters 100] [--warmup 20] [--out DIR]      -> DIR/eval_<W>x<H>.json (default profiles/)

The reference side is test.py:140-141,151 (the composition, three torch lines) followed by compute_errors as
tests/eval_ref.py restates it (reference_sequence: torch SSIM and PSNR with an .item() each, both images to the host, the
numpy norm, matplotlib's ScalarMappable over H W values, the upload) and test.py:186-187 (the RGBA ground truth); its SSIM
is the torch restatement oracle/losses.py.  Both sides are timed with device events around the whole call, alternating call
by call in one process; the median, p10 and p90 are reported in microseconds.  `kernel_only` times d3ga_eval_frames alone
inside a captured graph of 20 calls and forms its share of the HBM roofline from the bytes the algorithm has to move: 69 per
pixel with every output on (pred 12, image 12, alpha 4, boundary_fg 1 in; target 12, ground_truth 16, heat 12 out; the
partials are 12 bytes per 4096 pixels)."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_BYTES_PER_S = 8.0e12
SIZES = [(747, 1022), (1080, 1920)]                          # (W, H)
BYTES_PER_PIXEL = 12 + 12 + 4 + 1 + 12 + 16 + 12            # pred, image, alpha[0], boundary_fg bytes; target, ground_truth, heat


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    import eval_ref as er
    from d3ga_amd import Evaluator, _lib
    from oracle.losses import ssim as torch_ssim
    os.makedirs(a.out, exist_ok=True)
    for W, H in SIZES:
        pred, image, alpha, boundary = [torch.from_numpy(x[0]).cuda() for x in er.make_frame_inputs(W, 1, H, W, 3)]
        ev = Evaluator("white")

        def hip():
            return ev.add(pred, image, alpha, boundary)

        def reference():
            boundary_fg = 1.0 - boundary.float()                                             # test.py:140-141
            alpha_gt = alpha[0:1] * boundary_fg
            target = image * alpha_gt + (1 - alpha_gt) * 1.0                                 # :151
            heat, s, p = er.reference_sequence(target, pred, torch_ssim, lambda t: t.cuda())
            gt = torch.cat([image * alpha_gt, alpha_gt])                                     # :186-187
            return target, gt, heat, s, p

        with torch.no_grad():
            got, want = hip(), reference()
            torch.cuda.synchronize()
            er.check_heat(got["heatmap"].cpu().numpy(), got["target"].cpu().numpy(), pred.cpu().numpy())
            agree = {"target_max_abs": float((got["target"] - want[0]).abs().max()), "gt_max_abs": float((got["ground_truth"] - want[1]).abs().max()),
                     # as bytes, which is what the PNG writer stores: torch divides by a scalar as x * (1 / 255) on the device, one ulp
                     # beside the u8 / 255 of the reference's CPU run (and of this library) on two values in three
                     "heat_bytes_differing": int(((got["heatmap"] * 255).round() != (want[2] * 255).round()).any(0).sum()),
                     "heat_max_abs": float((got["heatmap"] - want[2]).abs().max()), "ssim_abs": abs(float(got["ssim"]) - want[3]),
                     "psnr_abs_db": abs(float(got["psnr"]) - want[4])}
            assert agree["target_max_abs"] <= 1e-6 and agree["gt_max_abs"] <= 1e-6 and agree["psnr_abs_db"] <= 1e-3 and agree["ssim_abs"] <= 1e-5, agree
            us = alternate({"hip": hip, "reference": reference}, a.iters, a.warmup)
        r = {n: stats(v) for n, v in us.items()}
        r["speedup_median"] = round(r["reference"]["median_us"] / r["hip"]["median_us"], 2)
        r["agreement"] = agree
        # kernel A alone, every output on
        L, p = _lib.lib(), lambda t: ctypes.c_void_p(t.data_ptr())
        target, heat, gt = torch.empty_like(pred), torch.empty_like(pred), torch.empty(4, H, W, device="cuda")
        partials = torch.empty(3 * L.d3ga_eval_partials(H, W), device="cuda")
        flags = _lib.EVAL_BG_WHITE | _lib.EVAL_ALPHA3

        def kernel_a():
            _lib.check(L.d3ga_eval_frames(1, H, W, flags, p(pred), p(image), p(alpha), p(boundary), p(target), p(gt), p(heat), p(partials),
                                          _lib.stream_handle()), "d3ga_eval_frames")

        k_us = graph_time(kernel_a)
        nbytes = BYTES_PER_PIXEL * W * H
        floor = nbytes / HBM_BYTES_PER_S * 1e6
        r["kernel_only"] = {"us": round(k_us, 2), "algorithmic_bytes": nbytes, "hbm_floor_us": round(floor, 2),
                            "roofline_share": round(floor / k_us, 3), "achieved_TBps": round(nbytes / k_us * 1e-6, 3),
                            "quads": bool((W * H) % 4 == 0)}
        r["all_kernels_us"] = round(graph_time(hip, calls=10), 2)                            # add() without the host: pointwise, SSIM, finish
        rec = {"size": [W, H], "B": 1, "iters": a.iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), **r}
        print(f"{W}x{H}: {json.dumps(r)}")
        json.dump(rec, open(os.path.join(a.out, f"eval_{W}x{H}.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
