"""ClipAdam (d3ga_amd/optim.py) against what it replaces -- `clip_grad_norm_(foreach=True)` + `torch.optim.Adam` -- on the
parameter lists of three shapes: the leaves of bench.Frame("C3") and of bench.Frame("C4") (SH colours), and the leaves of the
actor02-shaped ColorField step (`bench.py --train-step color`).  Gradients are filled once.  Device events around every call, the
two sides alternating call by call in one process; each both eager and as one captured graph (torch's Adam with
capturable=True there): median / p10 / p90 in microseconds.  "eager_moving": the eager step with the gradients at other
addresses on every call (two sets in turn), where ClipAdam rebuilds and uploads its tables every step -- the worst case of
an eager loop; a steady loop gets the same addresses back from the allocator and pays nothing.

    python tools/time_optim.py [--iters 100] [--warmup 20] [--out DIR]      -> DIR/optim_<shape>.json (default profiles/)
    python tools/time_optim.py --trace-target hip|torch --shape C3          20 eager steps of one side alone: the target of a
        `rocprofv3 --kernel-trace --stats -- python tools/time_optim.py --trace-target ...` run of its own (launches per step =
        calls / 20)

The update moves 7 dwords per element (read g, p, m, v; write p, m, v) and the norm one more: 32 bytes per element, set
against the 6.3 TB/s a float4 copy reaches on the MI355X.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
COPY_BYTES_PER_S = 6.3e12
BYTES_PER_ELEMENT = 32
SHAPES = ("C3", "C4", "color")


def leaf_shapes(shape, dev):
    """[(tensor shape, group)] of the trainable leaves; one param group per learning rate as the reference builds them."""
    import bench
    frame = bench.Frame("C4" if shape == "color" else shape, dev, 0)
    if shape != "color":
        return [(tuple(p.shape), i) for i, p in enumerate(frame.params.values())]
    frame.train_step(with_fields="color", pair=True, scale_weight=175.0)
    p = frame.params
    buckets = [list(frame.color_field.parameters()), [frame.color_feat], [frame.frame_enc], list(frame.canon_field.parameters()),
               [p["rotation"]], [p["scaling"]], list(frame.deform_field.parameters())]
    return [(tuple(q.shape), i) for i, b in enumerate(buckets) for q in b]


def make_side(kind, shapes, dev, captured, moving=False):
    from d3ga_amd.optim import ClipAdam
    gen = torch.Generator(device=dev).manual_seed(3)
    params = [torch.nn.Parameter(torch.randn(s, generator=gen, device=dev)) for s, _ in shapes]
    for q in params:
        q.grad = 0.01 * torch.randn(q.shape, generator=gen, device=dev)
    groups = [{"params": [q for q, (_, k) in zip(params, shapes) if k == j], "lr": 1e-4 * (1 + j)} for j in sorted({k for _, k in shapes})]
    if kind == "hip":
        opt = ClipAdam(groups, max_norm=2.5)
        fn = opt.step
    else:
        opt = torch.optim.Adam(groups, foreach=True, capturable=captured)

        def fn():
            torch.nn.utils.clip_grad_norm_(params, 2.5, foreach=True)
            opt.step()
    if moving:
        sets = [[q.grad for q in params], [q.grad.clone() for q in params]]
        turn, step = [0], fn

        def fn():
            turn[0] ^= 1
            for q, g in zip(params, sets[turn[0]]):
                q.grad = g
            step()
    if not captured:
        return fn, (opt, params)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    torch.cuda.synchronize()
    return graph.replay, (opt, params, graph)        # the graph reads the optimizer's buffers: all three stay alive


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles"))
    ap.add_argument("--shape", choices=SHAPES)
    ap.add_argument("--trace-target", choices=("hip", "torch"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda", 0)
    if a.trace_target:
        fn, _ = make_side(a.trace_target, leaf_shapes(a.shape or "C3", dev), dev, captured=False)
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        return
    os.makedirs(a.out, exist_ok=True)
    for shape in ([a.shape] if a.shape else SHAPES):
        shapes = leaf_shapes(shape, dev)
        torch.cuda.empty_cache()
        n = sum(int(np.prod(s)) for s, _ in shapes)
        rec = {"shape": shape, "n_tensors": len(shapes), "n_floats": n, "n_groups": len({k for _, k in shapes}), "iters": a.iters,
               "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "bytes_per_step_model": BYTES_PER_ELEMENT * n,
               "floor_us_at_copy_rate": round(BYTES_PER_ELEMENT * n / COPY_BYTES_PER_S * 1e6, 2)}
        for mode in ("eager", "eager_moving", "captured"):
            sides = {k: make_side(k, shapes, dev, captured=mode == "captured", moving=mode == "eager_moving") for k in ("torch", "hip")}
            us = alternate({k: v[0] for k, v in sides.items()}, max(a.iters, 100), max(a.warmup, 20))
            r = {k: stats(v) for k, v in us.items()}
            r["speedup_median"] = round(r["torch"]["median_us"] / r["hip"]["median_us"], 2)
            r["hip_p90_below_torch_p10"] = bool(r["hip"]["p90_us"] < r["torch"]["p10_us"])
            r["hip_bytes_per_s_model"] = round(BYTES_PER_ELEMENT * n / (r["hip"]["median_us"] * 1e-6), 0)
            r["hip_share_of_copy_rate"] = round(r["hip_bytes_per_s_model"] / COPY_BYTES_PER_S, 3)
            rec[mode] = r
            print(f"{shape} {mode}: hip {r['hip']} torch {r['torch']} x{r['speedup_median']} share of 6.3 TB/s {r['hip_share_of_copy_rate']}")
            del sides
            torch.cuda.empty_cache()
        json.dump(rec, open(os.path.join(a.out, f"optim_{shape}.json"), "w"), indent=1)
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
