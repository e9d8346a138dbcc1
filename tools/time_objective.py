"""The training objective (d3ga_amd/objective.py) against the torch lines it replaces, on the GPU: models/cage_net.py:214, 226
per cage and train.py:190-244 over the batch, in the float32 form of tests/objective_ref.py.  Device events around every
call, the two sides alternating call by call in one process: median / p10 / p90 in microseconds, forward and forward +
backward, at the actor02 shape (135 000 Gaussians in three cages, B = 1, poses on, blur off) and the C3 shape (500 000 in three
cages); the same inside a captured graph of 20 calls, one twentieth of a replay: what a call costs a replayed training step;
and `scale_energy` alone on one tensor of all the Gaussians.

    python tools/time_objective.py [--iters 200] [--warmup 30] [--out DIR]     -> DIR/objective_timing.json (default profiles/)

The events time the block as a user calls it (launches plus the Python layer's enqueue work); at these sizes the eager figures
are host time on both sides.  The torch side is charged with exp(scaling + delta_scale) because the product path never
materialises the activated scales (cage_deform(..., scale_activation="exp")); a trainer that keeps them for other reasons
pays less than the figure here."""
import argparse
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
from time_calib import alternate, graph_time, nograd, stats  # noqa: E402  (tools/ is the script's directory)

import objective_ref as R  # noqa: E402

SHAPES = {"actor02": 135_000, "C3": 500_000}
N_CAGES, N_DIMS, POSE_WIDTH = 3, 32, 87


def sides(P):
    from d3ga_amd.objective import TrainingObjective, scale_energy
    g = torch.Generator().manual_seed(P)
    per = P // N_CAGES
    scaling = [(-4.5 + 0.5 * torch.randn(per, 3, generator=g)).cuda().requires_grad_(True) for _ in range(N_CAGES)]
    delta = [(0.1 * torch.randn(per, 3, generator=g)).cuda().requires_grad_(True) for _ in range(N_CAGES)]
    fr = R.make_frames(1, N_CAGES, N_DIMS, POSE_WIDTH, fm=True, blur=False, vgg=False, seed=1, device="cuda", requires_grad=True)[0]
    small = [fr[k] for k in R.KEYS if fr[k] is not None and k != "scale_energy"]
    leaves = scaling + delta + small
    obj = TrainingObjective(**R.WEIGHTS)
    up = torch.ones((), device="cuda")

    def hip():
        e = torch.cat([scale_energy(s, d) for s, d in zip(scaling, delta)])
        return obj([dict(fr, scale_energy=e)])

    def aten():
        e = torch.cat([R.scale_energy(s, d, dtype=torch.float32) for s, d in zip(scaling, delta)])
        return R.objective([dict(fr, scale_energy=e)], R.WEIGHTS, torch.float32)[0]

    with torch.no_grad():
        a, b = float(hip()), float(aten())
    assert abs(a - b) <= 1e-5 * abs(b), (a, b)

    def fwd_bwd(fn):
        def run():
            for t in leaves:
                t.grad = None
            fn().backward(up)
        return run

    whole_s = torch.cat([s.detach() for s in scaling]).requires_grad_(True)
    whole_d = torch.cat([d.detach() for d in delta]).requires_grad_(True)

    def se(fn):
        def run():
            whole_s.grad = whole_d.grad = None
            fn(whole_s, whole_d).backward(up.reshape(1))
        return run
    se_hip, se_aten = (lambda s, d: scale_energy(s, d)), (lambda s, d: R.scale_energy(s, d, dtype=torch.float32))
    timed = {"objective_fwd": {"hip": nograd(hip), "aten": nograd(aten)},
             "objective_fwd_bwd": {"hip": fwd_bwd(hip), "aten": fwd_bwd(aten)},
             "scale_energy_fwd": {"hip": nograd(lambda: se_hip(whole_s, whole_d)), "aten": nograd(lambda: se_aten(whole_s, whole_d))},
             "scale_energy_fwd_bwd": {"hip": se(se_hip), "aten": se(se_aten)}}
    return timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    os.makedirs(a.out, exist_ok=True)
    rec = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "n_cages": N_CAGES, "n_dims": N_DIMS,
           "pose_width": POSE_WIDTH, "batch": 1, "shapes": {}}
    for name, P in SHAPES.items():
        timed = sides(P)
        r = {"gaussians": P}
        for what, fns in timed.items():
            us = alternate(fns, max(a.iters, 100), max(a.warmup, 20))
            r[what] = {k: stats(v) for k, v in us.items()}
            print(f"{name} {what}: hip {r[what]['hip']} aten {r[what]['aten']}", flush=True)
        r["in_graph_us"] = {what: {k: round(graph_time(fn), 2) for k, fn in fns.items()} for what, fns in timed.items()}
        print(f"{name} in a replayed graph, us per call: {r['in_graph_us']}", flush=True)
        rec["shapes"][name] = r
    json.dump(rec, open(os.path.join(a.out, "objective_timing.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
