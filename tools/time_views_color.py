"""The actor02-shaped colour step over a batch of k frames, view-batched against sequential.

configs/actorshq_actor02.yml (use_shs: false): every frame of the batch has its own pose (LBS + cage deform), its own camera, its own
ColorField colours and opacities (view direction and frame encoding, models/cage_net.py:232-258) and its own random background
(models/trainer.py:95-100); the losses of the batch are averaged (train.py:218-221).  Two forms of the same step:

    batched     ColorField per frame, then ONE renderer.render_views over the k packages -- per-frame geometry, rgb, opacity and
                background (d3ga_raster_params::per_view_geometry / per_view_appearance / per_view_background) -- with the RGB +
                silhouette pair, L1 on both images, the whole backward
    sequential  the same, with k renderer.render_pair calls (one camera per call, as the reference renders)

Each step is captured as one hipGraph (graph.CapturedStep) and replayed; every replay is timed with device events.  Printed: median,
p10 and p90 of ms per FRAME (step / k), for the whole step and for its render part alone (the same step with the deform and
ColorField outputs held fixed), and the agreement of the two forms (loss, gradients).  Last line: one JSON record.

    python tools/time_views_color.py [--workload C3] [--frames 4] [--steps 40] [--warmup 10]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(ms):
    a = np.asarray(ms)
    return {"median": round(float(np.median(a)), 4), "p10": round(float(np.percentile(a, 10)), 4), "p90": round(float(np.percentile(a, 90)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C3")
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_views_color.py measures on the GPU; no GPU found")
    import bench
    from d3ga_amd import rasterizer as R
    from d3ga_amd.cage_deform import lbs_cage_deform
    from d3ga_amd.cameras import batch_to_camera
    from d3ga_amd.graph import CapturedStep
    from d3ga_amd.losses import l1_loss
    from d3ga_amd.mlp import ColorField, view_directions
    from d3ga_amd.raster_views import CameraBatch
    from d3ga_amd.renderer import render_pair, render_views

    dev = torch.device("cuda")
    k = args.frames
    frame = bench.Frame(args.workload, dev, view_index=0)
    wl, p = frame.wl, frame.params
    P = frame.barys0.shape[0]
    rng = torch.Generator().manual_seed(7)
    torch.manual_seed(7)
    poses = [torch.from_numpy(frame.syn.pose_matrices(frame.joint_pos, np.random.default_rng(1000 + v))).to(dev) for v in range(k)]
    pose_vecs = [(0.3 * torch.randn(98, generator=rng)).to(dev) for _ in range(k)]          # the ColorField's pose input per frame
    batches = [frame.syn.make_batch(wl.width, wl.height, azimuth=2 * math.pi * v / max(8, k), camera_id=v, fill=frame.fill) for v in range(k)]
    W, H = int(batches[0]["width"]), int(batches[0]["height"])
    cams = CameraBatch(k, W, H, device=dev).set(batches)
    centres = [batch_to_camera(b, device=dev).camera_center.reshape(1, 3) for b in batches]
    targets = torch.stack([torch.rand(3, H, W, generator=torch.Generator().manual_seed(100 + v)) for v in range(k)]).to(dev)
    sil_t = (targets.mean(1, keepdim=True) > 0.5).float().expand(-1, 3, -1, -1).contiguous()
    bg = torch.rand(k, 3, generator=rng).to(dev)                      # models/trainer.py:95-100: a random background per frame
    sil_rgb, bg0 = torch.ones(P, 3, device=dev), torch.zeros(3, device=dev)
    color_field = ColorField().to(dev)
    color_feat = (0.33 * torch.rand(P, 64, generator=rng)).to(dev).requires_grad_(True)
    frame_enc = (0.1 * torch.randn(k, 32, generator=rng)).to(dev).requires_grad_(True)
    geo_params = [p["delta_node"], p["delta_bary"], p["scaling"], p["rotation"]]
    params = geo_params + list(color_field.parameters()) + [color_feat, frame_enc]

    def package(v):
        means, cov6, _ = lbs_cage_deform(frame.canon, p["delta_node"], poses[v], frame.skin_idx, frame.skin_w, frame.tetras, frame.tetra_id,
                                         frame.barys0, frame.canon_grad, p["scaling"], p["rotation"], delta_barys=p["delta_bary"],
                                         scale_activation="exp", gradient_per_tet=frame.canon_grad_mode == "per-tet")
        rgb, opac = color_field(color_feat, pose_vecs[v], view_directions(means, centres[v]), frame_encoding=frame_enc[v])
        return {"means3D": means, "cov3D_precomp": cov6, "opacities": opac, "rgb": rgb, "shs": None, "sh_degree": 0}

    # the render part alone: the same packages with their tensors held fixed (leaves) -- deform and ColorField out of the step
    with torch.no_grad():
        fixed = [{n: (t.detach().clone().requires_grad_(True) if torch.is_tensor(t) else t) for n, t in package(v).items()} for v in range(k)]
    fixed_params = [t for pk in fixed for t in pk.values() if torch.is_tensor(t)]

    def batched(pkgs):
        out = render_views(None, pkgs, bg, cameras=cams, colors2=sil_rgb, bg_color2=bg0)
        loss = l1_loss(out["render"].view(3 * k, H, W), targets.view(3 * k, H, W)) + l1_loss(out["render2"].view(3 * k, H, W), sil_t.view(3 * k, H, W))
        loss.backward()
        return loss

    def sequential(pkgs):
        tot = None
        for v in range(k):
            both = render_pair(batches[v], pkgs[v], bg[v], sil_rgb, bg0)
            loss = (l1_loss(both["render"], targets[v]) + l1_loss(both["render2"], sil_t[v])) / k
            loss.backward()
            tot = loss.detach() if tot is None else tot + loss.detach()
        return tot

    steps = {
        "batched": (lambda: batched([package(v) for v in range(k)]), params),
        "sequential": (lambda: sequential([package(v) for v in range(k)]), params),
        "batched_render_only": (lambda: batched(fixed), fixed_params),
        "sequential_render_only": (lambda: sequential(fixed), fixed_params),
    }
    res, grads = {}, {}
    for name, (fn, leaves) in steps.items():
        def zero():
            for q in leaves:
                q.grad = None
        R.set_capacity_policy("auto")
        for _ in range(3):
            zero(); fn()
        torch.cuda.synchronize()
        R.set_capacity_policy("static", int(R.last_counters()["D"] * 1.3) + 4096)
        zero(); fn()
        torch.cuda.synchronize()
        graph = CapturedStep(fn, params=leaves)
        for _ in range(args.warmup):
            graph.replay()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
        for e0, e1 in ev:
            e0.record()
            graph.replay()
            e1.record()
        torch.cuda.synchronize()
        graph.check_overflow()
        ms = [e0.elapsed_time(e1) / k for e0, e1 in ev]
        res[name] = dict(_stats(ms), loss=float(graph.result.detach()))
        grads[name] = [None if q.grad is None else q.grad.detach().clone() for q in leaves]
        print(f"{name:24s} ms per frame: median {res[name]['median']:.4f}  p10 {res[name]['p10']:.4f}  p90 {res[name]['p90']:.4f}  "
              f"(loss {res[name]['loss']:.6f})", flush=True)
        del graph
    R.set_capacity_policy("auto")

    def agree(a, b):
        return max(float((x - y).abs().max() / (y.abs().max() + 1e-30)) for x, y in zip(grads[a], grads[b]) if y is not None)
    out = {"workload": args.workload, "gaussians": P, "width": W, "height": H, "frames": k, "steps": args.steps, "warmup": args.warmup,
           "step": "per frame: LBS + cage deform, ColorField (rgb + opacity), RGB + silhouette render with a random background, L1 on both "
                   "images; losses averaged over the batch; whole backward; one hipGraph replay per step, timed with device events",
           "ms_per_frame": res,
           "speedup_step": round(res["sequential"]["median"] / res["batched"]["median"], 3),
           "speedup_render": round(res["sequential_render_only"]["median"] / res["batched_render_only"]["median"], 3),
           "loss_rel_diff": abs(res["batched"]["loss"] - res["sequential"]["loss"]) / abs(res["sequential"]["loss"]),
           "max_rel_gradient_difference": float(f"{agree('batched', 'sequential'):.2e}"),
           "max_rel_gradient_difference_render_only": float(f"{agree('batched_render_only', 'sequential_render_only'):.2e}")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
