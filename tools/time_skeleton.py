"""Forward + backward of `goliath_cage` per call at Goliath size (J = 160 joints, 104 pose + 29 scale parameters, V = 8000
cage vertices with 8 weights each), the HIP path (d3ga_amd/skeleton_model.py) against the same computation as float32 eager
torch ops on the same GPU (the one-joint-after-the-other solve and the gather / matmul skinning the reference runs).

One call = goliath_cage(module, motion, delta) and a backward from a random gradient on geom into motion and delta.  Timed with
device events around each call; before each timed call a spin kernel keeps the GPU busy while the host queues the work.
Printed: median / p10 / p90 ms per call for B = 1 and B = 4 (median of --steps calls after --warmup warm-ups), eager and as one
captured graph replayed (the eager HIP figure is dominated by the host queueing small launches), and the eager ratio.
Last line: one JSON record.  Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/time_skeleton.py
--hip-only` in a run of its own.

    python tools/time_skeleton.py [--frames 1 4] [--steps 100] [--warmup 20] [--hip-only]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
J, N_POSE, N_SCALE, V, K = 160, 104, 29, 8000, 8


def _stats(ms):
    a = np.asarray(ms)
    return {"median": round(float(np.median(a)), 4), "p10": round(float(np.percentile(a, 10)), 4),
            "p90": round(float(np.percentile(a, 90)), 4)}


def time_calls(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        torch.cuda._sleep(2_000_000)           # the GPU busy while the host queues the call
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def eager_cage(m, motion, delta, rot180):
    """goliath_cage's result as eager float32 torch ops, call for call what lib/blueman.py:101-168 runs."""
    from d3ga_amd import skeleton_model as sm
    lbs = m.lbs_fn
    B = motion.shape[0]

    def solve(scales):
        param = lbs.param_transform(torch.cat([motion, scales], 1))
        states = sm.solve_skeleton_state_torch(param, lbs.joint_offset, lbs.joint_rotation, lbs.joint_parents)
        return sm.states_to_matrix_torch(lbs.bind_state, states)
    template = (m.lbs_template_verts.expand(B, -1, -1) / 100.0 + delta.expand(B, -1, -1)) * 100.0
    mat = solve(m.lbs_scale.expand(B, -1))
    hom = torch.cat([template, torch.ones_like(template[..., :1])], 2)
    vs = torch.matmul(mat[:, lbs.skin_indices], hom[:, :, None, :, None])
    geom = (vs * lbs.skin_weights[None, :, :, None, None]).sum(2).squeeze(3) * m.global_scaling
    root = solve(torch.zeros(B, N_SCALE, device=motion.device))[:, 1]
    RT = torch.eye(4, device=motion.device)[None].repeat(B, 1, 1)
    RT[:, :3, :3] = root[:, :, :3]
    RT[:, :3, 3] = root[:, :, 3] / 1000.0
    RT = torch.linalg.inv(RT @ rot180)
    geom = geom / 1000
    return geom @ RT[:, :3, :3].transpose(1, 2) + RT[:, None, :3, 3], RT


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--hip-only", action="store_true")
    args = ap.parse_args()
    import goliath_ref as gr
    from d3ga_amd.skeleton_model import LBSModule, default_rot180, goliath_cage
    dev = "cuda:0"
    rng = np.random.default_rng(160)
    rig = gr.random_rig(rng, J, N_POSE, N_SCALE, kind="bushy", V=V, K=K, max_depth=20, t_mag=1.0)
    rest = rng.normal(size=(V, 3)).astype(np.float32) * 100
    m = LBSModule(gr.rig_json(rig.joint_offset.numpy(), rig.joint_rotation.numpy(), rig.parents, rig.skin_idx.numpy(),
                              rig.skin_w.numpy(), rest),
                  gr.rig_config(rig.transform.numpy(), rig.offsets.numpy(), N_POSE, N_SCALE), rest,
                  rng.uniform(-0.1, 0.1, size=(1, N_SCALE)).astype(np.float32), np.asarray([10.0], dtype=np.float32)).to(dev)
    depth = np.zeros(J, dtype=int)
    for j in range(1, J):
        depth[j] = depth[rig.parents[j]] + 1
    rec = {"tool": "time_skeleton", "J": J, "n_pose": N_POSE, "n_scale": N_SCALE, "V": V, "K": K, "levels": int(depth.max()) + 1,
           "transform_nonzeros": int(np.count_nonzero(rig.transform.numpy())), "device": torch.cuda.get_device_name(0),
           "steps": args.steps, "warmup": args.warmup, "cases": []}
    rot180 = default_rot180(dev)
    for B in args.frames:
        g = torch.Generator().manual_seed(B)
        motion = (0.5 * torch.randn(B, N_POSE, generator=g)).to(dev).requires_grad_(True)
        delta = (0.01 * torch.randn(1, V, 3, generator=g)).to(dev).requires_grad_(True)
        gout = torch.randn(B, V, 3, generator=g).to(dev)

        def hip_call():
            geom, _ = goliath_cage(m, motion, delta)
            torch.autograd.backward([geom], [gout], inputs=[motion, delta])

        def torch_call():
            geom, _ = eager_cage(m, motion, delta, rot180)
            torch.autograd.backward([geom], [gout], inputs=[motion, delta])

        with torch.no_grad():
            a, b = goliath_cage(m, motion, delta)[0], eager_cage(m, motion, delta, rot180)[0]
        case = {"B": B, "max_abs_difference_to_eager": float((a - b).abs().max()), "max_abs_geom": float(b.abs().max())}
        for name, fn in (("hip", hip_call),) + (() if args.hip_only else (("torch_f32_eager", torch_call),)):
            st = _stats(time_calls(fn, args.steps, args.warmup))
            case[f"{name}_ms"] = st
            print(f"B={B} {name:16s}: median {st['median']:.4f} ms  p10 {st['p10']:.4f}  p90 {st['p90']:.4f}", flush=True)
        # the same call as ONE captured graph: what is left when the host queues nothing between the kernels
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            hip_call()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            hip_call()
        st = _stats(time_calls(graph.replay, args.steps, args.warmup))
        case["hip_graph_ms"] = st
        print(f"B={B} {'hip (graph)':16s}: median {st['median']:.4f} ms  p10 {st['p10']:.4f}  p90 {st['p90']:.4f}", flush=True)
        if not args.hip_only:
            case["speedup"] = round(case["torch_f32_eager_ms"]["median"] / case["hip_ms"]["median"], 2)
            print(f"B={B} ratio eager / hip: {case['speedup']}", flush=True)
        rec["cases"].append(case)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
