"""The triangle-mesh rasterizer (d3ga_amd/mesh_render.py, csrc/mesh_raster.hip) on a 15000-triangle bumpy sphere standing in
for a cage, at 1920 x 1080, at the Goliath frame (747 x 1022) and as B = 6 at 1080p (one test.py frame's worth of renders).

    python tools/time_mesh_render.py [--reps 30] [--out DIR]      -> DIR/mesh_render_<W>x<H>_B<B>.json (default profiles/)

Each entry point is timed with device events around replays of a captured graph of 10 calls (median per call).  The stages
inside d3ga_mesh_rasterize (setup = clear + face setup + scan, coverage, resolve) are read from the kernel durations of a
profiled eager run, as are shade, maps and the vertex normals; where the profiler reports no kernels the stage table is left
out and only the entry points are reported.  The atomic count is the number of covering (pixel, face) pairs (tests/mesh_ref.py
counts them on the CPU): the coverage kernel issues at most that many 64-bit atomic mins, fewer where its plain load shows that
a key cannot win.  Achieved GB/s are formed from the bytes of DESIGN.md 4.4f:
    rasterize   36 B per pixel (8 clear, 8 key read, 20 fragment out) + 16 B per covering pair + 100 B per face
    shade       16 B per pixel + 12 B per covered pixel
    maps        36 B per pixel + 12 B per covered pixel
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
CASES = [(1920, 1080, 1), (747, 1022, 1), (1920, 1080, 6)]     # (W, H, B)
STAGES = {"setup": ("mesh_clear_kernel", "mesh_setup_kernel", "mesh_scan_kernel"), "coverage": ("mesh_coverage_kernel",),
          "resolve": ("mesh_resolve_kernel",), "shade": ("mesh_shade_kernel",), "maps": ("mesh_maps_kernel",),
          "vertex_normals": ("mesh_vertex_normals_kernel",)}


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
    from d3ga_amd import MeshCameras, Renderer, _lib
    os.makedirs(a.out, exist_ok=True)
    L, p = _lib.lib(), lambda t: ctypes.c_void_p(t.data_ptr())
    v, f = mr.sphere(100, 75, 7)
    assert len(f) == 15000
    counts = {}
    for W, H, B in CASES:
        row = mr._sphere_cam(H, W, 2.4, (0.3, 0.4, -1.0)).astype(np.float64)
        if (W, H) not in counts:
            fr = mr.rasterize_ref(v, f, row, H, W)
            counts[(W, H)] = (fr["fragments"], int(fr["covered"].sum()), fr["pix_to_face"])
        pairs, covered, want = counts[(W, H)]
        K = np.array([[row[12], 0, row[14]], [0, row[13], row[15]], [0, 0, 1]])
        cams = MeshCameras(np.repeat(row[None, :9].reshape(1, 3, 3), B, 0), np.repeat(row[None, 9:12], B, 0), K, (H, W))
        verts = torch.from_numpy(v).cuda()[None].repeat(B, 1, 1)
        faces = torch.from_numpy(f).cuda()
        r = Renderer()
        sc = r.scratch(cams, verts, faces)
        topo = r.topology(faces)
        V, F = verts.shape[1], topo.F
        image = torch.empty(B, H, W, 3, device="cuda")
        maps = tuple(torch.empty(B, H, W, c, device="cuda") for c in (3, 3, 1, 1))
        off, lists = topo.csr(V, verts.device)
        fd, bg = topo.faces(verts.device), (ctypes.c_float * 3)(1, 1, 1)
        calls = {
            "rasterize": lambda: _lib.check(L.d3ga_mesh_rasterize(B, V, F, H, W, p(verts), p(fd), p(cams.data), p(sc.raw), p(sc.pix_to_face), p(sc.zbuf),
                                                                  p(sc.bary), _lib.stream_handle()), "rasterize"),
            "shade": lambda: _lib.check(L.d3ga_mesh_shade_flat(B, V, F, H, W, p(verts), p(fd), None, p(cams.data), p(sc.pix_to_face), p(sc.bary), bg,
                                                               p(image), _lib.stream_handle()), "shade"),
            "vertex_normals": lambda: _lib.check(L.d3ga_mesh_vertex_normals(B, V, F, p(verts), p(fd), p(off), p(lists), p(sc.normals),
                                                                            _lib.stream_handle()), "vertex_normals"),
            "maps": lambda: _lib.check(L.d3ga_mesh_maps(B, V, F, H, W, p(verts), p(fd), p(sc.normals), p(cams.data), p(sc.pix_to_face), p(sc.bary),
                                                        *(p(t) for t in maps), _lib.stream_handle()), "maps"),
        }
        for fn in calls.values():
            fn()
        torch.cuda.synchronize()
        got = sc.pix_to_face[0].cpu().numpy()
        differ = int((got != want).sum())
        assert differ <= 0.02 * covered, (differ, covered)                  # the marginal pixels at most
        us = {k: round(graph_time(fn, reps=a.reps), 2) for k, fn in calls.items()}
        us["render"] = round(graph_time(lambda: r.render(cams, verts, faces, out=image, scratch=sc), reps=a.reps), 2)
        us["maps_call"] = round(graph_time(lambda: r.maps(cams, verts, faces, out=maps, scratch=sc), reps=a.reps), 2)

        def everything():
            for fn in calls.values():
                fn()

        try:
            stages = kernel_stages(everything)
        except Exception as e:                                            # a profiler that does not run here: entry points only
            stages = None
            print(f"no per-kernel stages: {type(e).__name__}: {e}")
        px = B * H * W
        nbytes = {"rasterize": 36 * px + 16 * B * pairs + 100 * B * F, "shade": 16 * px + 12 * B * covered, "maps": 36 * px + 12 * B * covered}
        rec = {"size": [W, H], "B": B, "faces": F, "vertices": V, "device": torch.cuda.get_device_name(0), "entry_points_us": us,
               "stages_us": stages, "covered_pixels_per_frame": covered, "atomic_candidates_per_frame": pairs,
               "pixels_differing_from_the_oracle": differ, "algorithmic_bytes": nbytes,
               "achieved_GBps": {k: round(nbytes[k] / us[k] * 1e-3, 1) for k in nbytes}}
        print(f"{W}x{H} B={B}: {json.dumps(rec)}")
        json.dump(rec, open(os.path.join(a.out, f"mesh_render_{W}x{H}_B{B}.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
