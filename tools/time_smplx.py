"""Forward + backward of the SMPL-X body model per call at SMPL-X size (V = 10475, J = 55, 486 pose features), the HIP layer
(d3ga_amd/body_model.py) against the float32 eager torch restatement of the oracle (tests/smplx_ref.py) on the same GPU.

One call = layer(poses, shapes, Rh, Th, expression) and a backward from random gradients on all four outputs into poses,
shapes, expression, Rh and Th.  Timed with device events around each call, on a synthetic model (d3ga_amd.synthetic).
Two cache states:
    warm   calls back to back: the 61 MB of posedirs stay resident in the 256 MiB Infinity Cache between calls
    cold   a 512 MiB buffer is overwritten before every call, so the blend directions come from HBM
Before each timed call the stream is kept busy (a spin kernel after the overwrite, if any) while the host queues the call, so the
events bound the call's GPU work and not the host's launch overhead.
Printed: median / p10 / p90 ms per call, the algorithmic bytes per call and the fraction of 6.3 TB/s they imply.  Last
line: one JSON record.

    python tools/time_smplx.py [--frames 1 4] [--steps 50] [--warmup 10]
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_TBPS = 6.3


def _stats(ms):
    a = np.asarray(ms)
    return {"median": round(float(np.median(a)), 4), "p10": round(float(np.percentile(a, 10)), 4),
            "p90": round(float(np.percentile(a, 90)), 4)}


def algorithmic_bytes(layer, B):
    """Bytes a fused forward + backward must move: the blend directions read twice, the template and the skinning CSR twice,
    the outputs written once (verts, T, A, bs), T and bs read back, the four upstream gradients read."""
    nr = layer.n_shape + layer.n_expr + 9 * (layer.J - 1)
    V, J = layer.V, layer.J
    nnz = int(layer.bm_w_val.numel())
    model = 2 * (nr * 3 * V * 4 + V * 12 + nnz * 8 + (V + 1) * 4)
    outs = B * (V * (12 + 64 + 12) + J * 64) * 4
    back = B * V * (64 + 12) * 4 + B * (V * (12 + 64 + 12) + J * 64) * 4
    return model + outs + back


def time_calls(fn, steps, warmup, flush=None):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        if flush is not None:
            flush.add_(1.0)
        torch.cuda._sleep(2_000_000)           # the GPU busy while the host queues the call: events time kernels, not launches
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    from d3ga_amd import synthetic as syn
    from d3ga_amd.body_model import SMPLlayer
    from smplx_ref import RefSMPL
    dev = "cuda:0"
    data = syn.smpl_model_data("smplx", seed=11)
    with tempfile.TemporaryDirectory() as d:
        path = syn.write_smpl_model(os.path.join(d, "SMPLX_NEUTRAL.npz"), data)
        layer = SMPLlayer(path, model_type="smplx", gender="neutral").to(dev)
    ref = RefSMPL(data, dtype=torch.float32, device=dev)
    flush = torch.zeros(128 * 1024 * 1024, device=dev)          # 512 MiB: twice the Infinity Cache
    rec = {"tool": "time_smplx", "V": layer.V, "J": layer.J, "pose_features": 9 * (layer.J - 1),
           "device": torch.cuda.get_device_name(0), "hbm_tbps_assumed": HBM_TBPS, "cases": []}
    for B in args.frames:
        g = torch.Generator().manual_seed(B)
        poses = (0.35 * torch.randn(B, layer.NUM_POSES, generator=g)).to(dev).requires_grad_(True)
        shapes = torch.randn(B, 10, generator=g).to(dev).requires_grad_(True)
        expr = torch.randn(B, 10, generator=g).to(dev).requires_grad_(True)
        Rh = (0.5 * torch.randn(B, 3, generator=g)).to(dev).requires_grad_(True)
        Th = torch.randn(B, 3, generator=g).to(dev).requires_grad_(True)
        ups = [torch.randn(s, generator=g).to(dev) for s in ((B, layer.V, 3), (B, layer.V, 4, 4), (B, layer.J, 4, 4), (B, layer.V, 3))]
        ins = (poses, shapes, expr, Rh, Th)

        def hip_call():
            out = layer(poses=poses, shapes=shapes, Rh=Rh, Th=Th, expression=expr)
            torch.autograd.backward(out, ups, inputs=list(ins))

        def torch_call():
            out = ref(poses, shapes, Rh=Rh, Th=Th, expression=expr)
            torch.autograd.backward(out, ups, inputs=list(ins))

        nbytes = algorithmic_bytes(layer, B)
        case = {"B": B, "algorithmic_bytes": nbytes}
        for name, fn, steps in (("hip", hip_call, args.steps), ("torch_f32_eager", torch_call, max(5, args.steps // 5))):
            for state, fl in (("warm", None), ("cold", flush)):
                ms = time_calls(fn, steps, min(args.warmup, steps), fl)
                st = _stats(ms)
                st["hbm_fraction"] = round(nbytes / (st["median"] * 1e-3) / (HBM_TBPS * 1e12), 4)
                case[f"{name}_{state}_ms"] = st
                print(f"B={B} {name:16s} {state}: median {st['median']:.4f} ms  p10 {st['p10']:.4f}  p90 {st['p90']:.4f}  "
                      f"{nbytes / 1e6:.1f} MB -> {100 * st['hbm_fraction']:.1f}% of {HBM_TBPS} TB/s", flush=True)
        case["speedup_warm"] = round(case["torch_f32_eager_warm_ms"]["median"] / case["hip_warm_ms"]["median"], 2)
        case["speedup_cold"] = round(case["torch_f32_eager_cold_ms"]["median"] / case["hip_cold_ms"]["median"], 2)
        rec["cases"].append(case)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
