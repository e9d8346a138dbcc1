"""Barycentric attribute interpolation (d3ga_amd/bary_interp.py) against the torch formulation of the reference lines it
replaces, on the GPU: `einsum("ikj,ik->ij", attr[cells][cell_id], barys + delta_bary)` with int64 index buffers as the reference
registers them (models/cage_net.py:236-241,270; models/mesh_net.py:193).  Device events around every call, the two sides
alternating call by call in one process (tools/time_calib.py: alternate): median / p10 / p90 in microseconds, forward and
forward + backward, at
    actor02         P = 135 000, K = 4: C = 1 through a many-to-one map onto 10 475 body vertices (the shadow column), and C = 3
                    on the cage's own vertices (canonical means) -- the binding of synthetic workload C4
    mesh            P = 135 000, K = 3, C = 3, V = 10 475 (the mesh primitive's means; a synthetic coherent triangle strip)
    C3              P = 500 000, K = 4, C = 3 -- the binding of synthetic workload C3

    python tools/time_bary_interp.py [--iters 200] [--warmup 30] [--out FILE]     -> profiles/bary_interp_timing.json

The events time the op as a user calls it (launches plus the Python layer's enqueue work).  `kernel_only` times the HIP op again
inside a captured graph of 20 calls, one twentieth of a replay: the kernels without the host, which is what the share of the HBM
roofline is formed from.  Algorithmic bytes (every stream once, the gathered table once):
    forward    P (8 K [+ 4 K with delta] + 4 C) + 4 V C
    backward   g_barys: P (8 K + 4 C) + 4 V C;  g_attr: 4 K P items + P (4 K [+ 4 K]) weights + 4 P C + 4 V C written + 4 (V + 1)"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from time_calib import HBM_BYTES_PER_S, alternate, fwd_bwd, graph_time, nograd, stats  # noqa: E402

BODY_VERTICES = 10_475


def fwd_bytes(P, K, C, V, delta=True):
    return P * (8 * K + (4 * K if delta else 0) + 4 * C) + 4 * V * C


def bwd_bytes(P, K, C, V, delta=True):
    g_barys = P * (8 * K + 4 * C) + 4 * V * C
    g_attr = 4 * K * P + P * (4 * K + (4 * K if delta else 0)) + 4 * P * C + 4 * V * C + 4 * (V + 1)
    return g_barys + g_attr


def cage_shapes(workload, dev):
    """The binding of a synthetic workload -> (tetras, tetra_id int64, barys, canonical cage points)."""
    from d3ga_amd import synthetic as syn
    sc = syn.make_scene(workload)
    return sc["tetras"].long().to(dev), sc["tetra_id"].long().to(dev), sc["barys"].float().to(dev), sc["canon_points"].float().to(dev)


def mesh_shapes(P, V, dev, g):
    """A coherent strip of 2 V triangles over V vertices, the Gaussians sorted by face -> face ids (P,3) int64, barys (P,3)."""
    f = torch.sort(torch.randint(0, 2 * V, (P,), generator=g))[0]
    face_ids = torch.stack([f // 2, (f // 2 + 1 + f % 2) % V, (f // 2 + 103) % V], 1)
    barys = torch.rand(P, 3, generator=g)
    return face_ids.to(dev), (barys / barys.sum(1, keepdim=True)).to(dev)


def sides(attr, barys, delta, up, hip_binding, gather):
    """gather(attr) -> (P,K,C): the reference's indexing chain.  -> the timed callables of both sides and of the graph timing"""
    from d3ga_amd.bary_interp import bary_interp
    hip = lambda: bary_interp(attr, hip_binding, barys, delta)
    aten = lambda: torch.einsum("ikj,ik->ij", gather(attr), barys + delta)
    with torch.no_grad():
        err = float((hip() - aten()).abs().max())
    assert err <= 1e-5 * max(1.0, float(attr.detach().abs().max())), err
    leaves = (attr, delta)
    return ({"fwd": {"hip": nograd(hip), "aten": nograd(aten)},
             "fwd_bwd": {"hip": fwd_bwd(hip, leaves, up), "aten": fwd_bwd(aten, leaves, up)}},
            {"fwd": nograd(hip), "fwd_bwd": fwd_bwd(hip, leaves, up)})


def record(name, timed, kernels, shape, a):
    P, K, C, V = (shape[k] for k in "PKCV")
    rec = dict(shape, iters=a.iters, warmup=a.warmup)
    for what, fns in timed.items():
        us = alternate(fns, max(a.iters, 100), max(a.warmup, 20))
        rec[what] = {n: stats(v) for n, v in us.items()}
        rec[what]["speedup_median"] = round(rec[what]["aten"]["median_us"] / rec[what]["hip"]["median_us"], 2)
        print(f"{name} {what}: hip {rec[what]['hip']} aten {rec[what]['aten']} x{rec[what]['speedup_median']}")
    rec["kernel_only"] = {}
    for what, fn in kernels.items():
        nbytes = fwd_bytes(P, K, C, V) + (bwd_bytes(P, K, C, V) if what == "fwd_bwd" else 0)
        us = graph_time(fn)
        floor = nbytes / HBM_BYTES_PER_S * 1e6
        rec["kernel_only"][what] = {"us": round(us, 2), "algorithmic_bytes": nbytes, "hbm_floor_us": round(floor, 2),
                                    "roofline_share": round(floor / us, 3)}
        print(f"{name} kernel_only {what}: {rec['kernel_only'][what]}")
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bary_interp_timing.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    from d3ga_amd.bary_interp import BaryBinding
    dev = "cuda"
    g = torch.Generator().manual_seed(7)
    rand = lambda *s: torch.randn(*s, generator=g).to(dev)
    result = {"device": torch.cuda.get_device_name(0), "hbm_bytes_per_s": HBM_BYTES_PER_S, "shapes": {}}

    def cage(name, workload, with_shadow):
        tetras, tetra_id, barys, canon = cage_shapes(workload, dev)
        P, V = tetra_id.shape[0], canon.shape[0]
        delta = (0.05 * torch.tanh(rand(P, 4))).requires_grad_(True)
        if with_shadow:
            vmap = torch.randint(0, BODY_VERTICES, (V,), generator=g).to(dev)
            ao = torch.rand(BODY_VERTICES, generator=g).to(dev).requires_grad_(True)
            b = BaryBinding(cells=tetras, cell_id=tetra_id, vertex_map=vmap, n_rows=BODY_VERTICES)
            timed, kernels = sides(ao, barys, delta, rand(P, 1), b, lambda t: t[vmap][..., None][tetras][tetra_id])
            result["shapes"][f"{name}_shadow_C1"] = record(f"{name} shadow", timed, kernels,
                                                           dict(P=P, K=4, C=1, V=BODY_VERTICES, cage_vertices=V), a)
        pts = canon.clone().requires_grad_(True)
        b = BaryBinding(cells=tetras, cell_id=tetra_id, n_rows=V)
        timed, kernels = sides(pts, barys, delta, rand(P, 3), b, lambda t: t[tetras][tetra_id])
        result["shapes"][f"{name}_points_C3"] = record(f"{name} points", timed, kernels, dict(P=P, K=4, C=3, V=V), a)

    cage("actor02", "C4", True)
    P = 135_000
    face_ids, barys = mesh_shapes(P, BODY_VERTICES, dev, g)
    pts = (0.4 * rand(BODY_VERTICES, 3)).requires_grad_(True)
    delta = (0.05 * torch.tanh(rand(P, 3))).requires_grad_(True)
    timed, kernels = sides(pts, barys, delta, rand(P, 3), BaryBinding(face_ids, n_rows=BODY_VERTICES), lambda t: t[face_ids])
    result["shapes"]["mesh_C3"] = record("mesh", timed, kernels, dict(P=P, K=3, C=3, V=BODY_VERTICES), a)
    cage("C3", "C3", False)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(result, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
