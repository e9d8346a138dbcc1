"""Time the backward of the skinned cage deformation (lbs_cage_deform, and lbs_cage alone) with and without the pose gradients
(dL/d(joint_mats, Rh, Th)), against the float32 eager-torch restatement of the skinning (oracle.deform.lbs_cage on the GPU).

    python tools/time_lbs_pose.py [--workload C3] [--iters 200]            -> one JSON line per configuration

Configurations: the workload's own skinning (C3: K = 4 over J = 55) and a Goliath-like one (J = 160, K = 8, indices drawn at
random on the same cage).  Each figure is the median over `--iters` of one backward (torch.autograd.grad with the graph
retained), bracketed by HIP events, after 20 warm-up calls.  Per-kernel times: run under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from d3ga_amd import synthetic as syn  # noqa: E402
from d3ga_amd.cage_deform import canonical_gradient, cage_deform, lbs_cage, lbs_cage_deform  # noqa: E402
from oracle import deform as od  # noqa: E402

DEV = "cuda:0"


def median_ms(fn, iters):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def run(sc, J, K, idx, w, A, iters, label):
    g = torch.Generator().manual_seed(1)
    d = lambda t: t.to(DEV)
    V, P = sc["canon_points"].shape[0], sc["barys"].shape[0]
    tmpl, tet, tid, bar = d(sc["canon_points"]), d(sc["tetras"]).int(), d(sc["tetra_id"]).int(), d(sc["barys"])
    cg = canonical_gradient(sc["canon_points"], sc["tetras"], sc["tetra_id"]).contiguous().to(DEV)
    scl, rot = d(sc["scaling"]), d(sc["rotation"])
    Rh = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))[0].float().to(DEV)
    Th = torch.randn(3, generator=g).to(DEV)
    gm, gc = torch.randn(P, 3, generator=g).to(DEV), torch.randn(P, 6, generator=g).to(DEV)
    gt = torch.randn(V, 3, generator=g).to(DEV)
    out = {"config": label, "V": V, "P": P, "J": J, "K": K}
    for pose in (False, True):
        delta = d(sc["delta_node"]).clone().requires_grad_(True)
        Al, Rl, Tl = (A.clone().requires_grad_(True), Rh.clone().requires_grad_(True), Th.clone().requires_grad_(True)) if pose \
            else (A, Rh, Th)
        ins = [delta] + ([Al, Rl, Tl] if pose else [])
        m, c, tp = lbs_cage_deform(tmpl, delta, Al, idx, w, tet, tid, bar, cg, scl, rot, scale_activation="exp", Rh=Rl, Th=Tl)
        loss = (m * gm).sum() + (c * gc).sum() + (tp * gt).sum()
        out[f"fused_bwd_ms_pose{int(pose)}"] = median_ms(lambda: torch.autograd.grad(loss, ins, retain_graph=True), iters)
        tp2 = lbs_cage(tmpl, delta, Al, idx, w, Rl, Tl)
        loss2 = (tp2 * gt).sum()
        out[f"lbs_bwd_ms_pose{int(pose)}"] = median_ms(lambda: torch.autograd.grad(loss2, ins, retain_graph=True), iters)
        if pose:                                                     # the float32 eager-torch restatement of the skinning
            tp3 = od.lbs_cage(tmpl, delta, Al, idx.long(), w, Rl, Tl)
            loss3 = (tp3 * gt).sum()
            out["eager_torch_lbs_bwd_ms_pose1"] = median_ms(lambda: torch.autograd.grad(loss3, ins, retain_graph=True), iters)
            m4, c4 = cage_deform(tp3, tet, tid, bar, cg, scl, rot, scale_activation="exp")
            loss4 = (m4 * gm).sum() + (c4 * gc).sum() + (tp3 * gt).sum()
            out["eager_torch_lbs_then_cage_deform_bwd_ms_pose1"] = median_ms(
                lambda: torch.autograd.grad(loss4, ins, retain_graph=True), iters)
    out["fused_added_us"] = 1000 * (out["fused_bwd_ms_pose1"] - out["fused_bwd_ms_pose0"])
    out["lbs_added_us"] = 1000 * (out["lbs_bwd_ms_pose1"] - out["lbs_bwd_ms_pose0"])
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C3")
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    sc = syn.make_scene(a.workload)
    A = sc["joint_mats"].to(DEV)
    run(sc, A.shape[0], sc["skin_idx"].shape[1], sc["skin_idx"].to(DEV).int(), sc["skin_w"].to(DEV), A, a.iters, f"{a.workload} own skinning")
    g = torch.Generator().manual_seed(2)
    V, J, K = sc["canon_points"].shape[0], 160, 8
    idx = torch.randint(0, J, (V, K), generator=g).int().to(DEV)
    w = torch.rand(V, K, generator=g)
    w = (w / w.sum(1, keepdim=True)).to(DEV)
    Ag = (torch.eye(4).repeat(J, 1, 1) + 0.1 * torch.randn(J, 4, 4, generator=g)).to(DEV)
    run(sc, J, K, idx, w, Ag, a.iters, f"{a.workload} Goliath-like J=160 K=8")


if __name__ == "__main__":
    main()
