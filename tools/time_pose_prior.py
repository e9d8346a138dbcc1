"""The pose prior (d3ga_amd/pose_prior.py) against the detour it replaces, on the GPU: the reference's per-frame PCA clamp
(test.py:88-92: `.cpu().numpy()`, scikit-learn `transform`, the clip, `inverse_transform`, `as_tensor(...).cuda().float()`) at
87 pose parameters and 30 components, and `PCA(n_components).fit` on the host against `PosePCA.fit` of a table that already
lives on the device.  The two sides alternate call by call in one process: median / p10 / p90.

    python tools/time_pose_prior.py [--iters 200] [--warmup 30] [--out DIR]     -> DIR/pose_prior_timing.json (default profiles/)

`clamp`: device events around every call (launch plus the Python layer's enqueue work on one side; two copies, a
synchronisation and scikit-learn on the other).  `in_graph_us`: the HIP call again inside a captured graph of 20 calls, one
twentieth of a replay -- the detour has no such figure, it cannot be captured.  `trajectory`: 2000 poses in one launch.  `fit`:
wall-clock milliseconds including the read-back and the host eigen-solve (both sides end on the host).  Needs scikit-learn for
the reference sides only; the product never imports it."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from time_calib import alternate, graph_time, stats  # noqa: E402  (tools/ is the script's directory)

D, K, SIGMA = 87, 30, 2.0
FITS = [(2_000, 87, 30), (20_000, 165, 30)]
TRAJECTORY = 2_000


def poses_table(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, d, generator=g) * (0.05 + torch.rand(d, generator=g)) + torch.randn(d, generator=g)).float()


def wall_alternate(fns, iters, warmup):
    """name -> ms per call (array), wall clock with a synchronisation behind every call"""
    out = {n: [] for n in fns}
    for i in range(warmup + iters):
        for n, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= warmup:
                out[n].append((time.perf_counter() - t0) * 1e3)
    return {n: np.array(v) for n, v in out.items()}


def ms_stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "p10_ms": round(float(np.percentile(ms, 10)), 3),
            "p90_ms": round(float(np.percentile(ms, 90)), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    from sklearn.decomposition import PCA
    from d3ga_amd.pose_prior import PosePCA
    os.makedirs(a.out, exist_ok=True)
    rec = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "pose_width": D, "n_components": K,
           "sigma": SIGMA}

    host = poses_table(2_000, D, 1)
    table = host.cuda()
    sk = PCA(n_components=K).fit(host.numpy())
    pca = PosePCA.fit(table, K)
    frame = {"smplx": {"poses": table[7:8].clone()}}
    std = np.sqrt(sk.explained_variance_)

    def detour():                                            # test.py:49-56, 88-92
        poses = frame["smplx"]["poses"].cpu().numpy()[0]
        low = sk.transform(poses.reshape(1, -1))
        low = np.minimum(np.maximum(low, -SIGMA * std), SIGMA * std)
        return torch.as_tensor(sk.inverse_transform(low)[0]).cuda().float()

    slot = torch.empty(1, D, device="cuda")
    cell = torch.tensor([7], dtype=torch.int32, device="cuda")
    hip = lambda: pca.clamp(frame["smplx"]["poses"], SIGMA, out=slot)
    hip_rows = lambda: pca.clamp_rows(table, cell, SIGMA, out=slot)
    assert float((hip()[0] - detour()).abs().max()) <= 1e-4
    us = alternate({"hip": hip, "hip_rows": hip_rows, "reference": detour}, max(a.iters, 100), max(a.warmup, 20))
    rec["clamp"] = {k: stats(v) for k, v in us.items()}
    rec["clamp"]["in_graph_us"] = {"hip": round(graph_time(hip), 2), "hip_rows": round(graph_time(hip_rows), 2)}
    print("clamp, one frame:", rec["clamp"])

    traj = table[:TRAJECTORY].contiguous()
    traj_out = torch.empty_like(traj)
    traj_host = host[:TRAJECTORY].numpy()

    def sk_traj():                                           # the same clamp over a whole sequence, poses on the host already
        low = sk.transform(traj_host)
        low = np.minimum(np.maximum(low, -SIGMA * std), SIGMA * std)
        return torch.as_tensor(sk.inverse_transform(low)).cuda().float()
    us = alternate({"hip": lambda: pca.clamp(traj, SIGMA, out=traj_out), "reference": sk_traj}, max(a.iters, 100), max(a.warmup, 20))
    rec["trajectory"] = {"poses": TRAJECTORY, **{k: stats(v) for k, v in us.items()}}
    print("trajectory:", rec["trajectory"])

    rec["fit"] = {}
    for n, d, k in FITS:
        h = poses_table(n, d, n)
        t = h.cuda()
        hn = h.numpy()
        ms = wall_alternate({"hip": lambda: PosePCA.fit(t, k), "reference": lambda: PCA(n_components=k).fit(hn)},
                            max(a.iters // 10, 10), 3)
        rec["fit"][f"{n}x{d}"] = {"n_components": k, **{name: ms_stats(v) for name, v in ms.items()}}
        print(f"fit {n} x {d}:", rec["fit"][f"{n}x{d}"])
    json.dump(rec, open(os.path.join(a.out, "pose_prior_timing.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
