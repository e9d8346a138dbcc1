"""The point-cloud view (d3ga_amd/point_render.py, csrc/point_raster.hip) on 135 000 points standing in for the Gaussian centres
of the C4 avatar and on the 500 000 of C3, at the Goliath frame (747 x 1022) and at 1080p, with the reference's settings
(radius 0.007, 5 points per pixel).

    python tools/time_point_render.py [--reps 30] [--out DIR]      -> DIR/point_render_<W>x<H>_P<P>.json (default profiles/)

The points fill a standing ellipsoid (a body's proportions: half axes 0.35, 0.9, 0.25 m) seen from 3 m so that it spans about
85 % of the frame's height; consecutive points are neighbours in space, as Gaussians stored in tetrahedron order are.  Each
entry point is timed with device events around replays of a captured graph of 10 calls (median per call).  The stages inside
d3ga_points_rasterize (binning = clear + count + the two scans + scatter; tiles) are read from the kernel durations of a
profiled eager run, as is the composite; where the profiler reports no kernels the stage table is left out and only the entry
points are reported.  Achieved GB/s are formed from the bytes of DESIGN.md 4.4h:
    rasterize   12 K B per pixel (fragments out) + 24 B per point (read twice) + 32 B per list record (written, read)
    composite   (8 K + 12) B per pixel
No ratio to the reference is formed: pytorch3d has no ROCm build."""
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
CASES = [(747, 1022, 135000), (1920, 1080, 135000), (747, 1022, 500000), (1920, 1080, 500000)]     # (W, H, P)
STAGES = {"binning": ("points_clear_kernel", "points_count_kernel", "points_local_kernel", "points_scan_kernel", "points_scatter_kernel"),
          "tiles": ("points_tile_kernel",), "composite": ("points_composite_kernel",)}


def graph_time(fn, calls=10, reps=30):
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
    for _ in range(3):
        g.replay()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        g.replay()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev])) * 1e3 / calls


def body_cloud(P, seed=5):
    """P points inside a standing ellipsoid, sorted along a space-filling order of 8 cm cells (neighbours in memory are
    neighbours in space) -> (P,3) float32"""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((P, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    x = d * np.cbrt(rng.random(P))[:, None] * [0.35, 0.9, 0.25]
    cell = np.floor((x + 1.0) / 0.08).astype(np.int64)
    return x[np.lexsort((cell[:, 0], cell[:, 2], cell[:, 1]))].astype(np.float32)


def kernel_stages(fn, iters=5):
    """us per stage and call from the profiler's kernel records, or None."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    total = {k: 0.0 for k in STAGES}
    seen = 0
    for e in prof.events():
        for stage, names in STAGES.items():
            if any(n in e.name for n in names) and getattr(e, "device_time", 0):
                total[stage] += e.device_time
                seen += 1
    return {k: round(v / iters, 2) for k, v in total.items()} if seen else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    import mesh_ref as mr
    from d3ga_amd import MeshCameras, PCRenderer, _lib
    os.makedirs(a.out, exist_ok=True)
    L, p = _lib.lib(), lambda t: ctypes.c_void_p(t.data_ptr())
    clouds = {}
    for W, H, P in CASES:
        if P not in clouds:
            clouds[P] = torch.from_numpy(body_cloud(P)).cuda()[None]
        verts = clouds[P]
        R, t = mr.look_at((0.6, 0.2, -2.9))
        f = 0.85 * H * 3.0 / 1.8                              # 1.8 m of body over 85 % of the rows, from 3 m
        Km = np.array([[f, 0, 0.5 * W + 0.3], [0, f, 0.5 * H - 0.2], [0, 0, 1]])
        cams = MeshCameras(R, t, Km, (H, W))
        r = PCRenderer()
        K, radius = r.points_per_pixel, r.radius
        sc = r.scratch(cams, verts)
        image = torch.empty(1, H, W, 3, device="cuda")
        colours = torch.rand(1, P, 3, device="cuda")
        bg = (ctypes.c_float * 3)(1, 1, 1)
        calls = {
            "rasterize": lambda: _lib.check(L.d3ga_points_rasterize(1, P, H, W, K, radius, p(verts), p(cams.data), p(sc.raw), p(sc.idx), p(sc.zbuf),
                                                                    p(sc.dists), _lib.stream_handle()), "rasterize"),
            "composite": lambda: _lib.check(L.d3ga_points_composite(1, P, H, W, K, radius, p(sc.idx), p(sc.dists), p(colours), bg, p(image),
                                                                    _lib.stream_handle()), "composite"),
        }
        for fn in calls.values():
            fn()
        torch.cuda.synchronize()
        idx = sc.idx[0]
        covered = int((idx[..., 0] >= 0).sum())
        full = int((idx[..., K - 1] >= 0).sum())
        # the list records: every point's tile rectangle, recomputed from its projection as the kernels cut it
        vc = verts[0].double() @ torch.from_numpy(R).cuda().T + torch.from_numpy(t).cuda()
        u, v = f * vc[:, 0] / vc[:, 2] + Km[0, 2], f * vc[:, 1] / vc[:, 2] + Km[1, 2]
        rb = radius * min(H, W) / 2 * 1.001 + 0.01
        i0, i1 = torch.ceil(u - rb - 0.5).clamp(0, W - 1), torch.floor(u + rb - 0.5).clamp(0, W - 1)
        j0, j1 = torch.ceil(v - rb - 0.5).clamp(0, H - 1), torch.floor(v + rb - 0.5).clamp(0, H - 1)
        ok = (i0 <= i1) & (j0 <= j1) & (vc[:, 2] > 0.01)
        records = int((((i1 // 16 - i0 // 16 + 1) * (j1 // 16 - j0 // 16 + 1))[ok]).sum())
        us = {k: round(graph_time(fn, reps=a.reps), 2) for k, fn in calls.items()}
        us["render"] = round(graph_time(lambda: r.render(cams, verts, colours, out=image, scratch=sc), reps=a.reps), 2)

        def everything():
            for fn in calls.values():
                fn()

        try:
            stages = kernel_stages(everything)
        except Exception as e:                                            # a profiler that does not run here: entry points only
            stages = None
            print(f"no per-kernel stages: {type(e).__name__}: {e}")
        px = H * W
        nbytes = {"rasterize": 12 * K * px + 24 * P + 32 * records, "composite": (8 * K + 12) * px}
        rec = {"size": [W, H], "B": 1, "points": P, "points_per_pixel": K, "radius": radius, "radius_px": round(radius * min(H, W) / 2, 3),
               "device": torch.cuda.get_device_name(0), "entry_points_us": us, "stages_us": stages, "covered_pixels": covered,
               "pixels_with_all_slots_filled": full, "list_records": records, "pixel_point_tests": records * 256,
               "scratch_bytes": int(sc.raw.numel()), "algorithmic_bytes": nbytes,
               "achieved_GBps": {k: round(nbytes[k] / us[k] * 1e-3, 1) for k in nbytes}}
        print(f"{W}x{H} P={P}: {json.dumps(rec)}")
        json.dump(rec, open(os.path.join(a.out, f"point_render_{W}x{H}_P{P}.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
