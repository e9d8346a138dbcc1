"""Gaussian initialisation (d3ga_amd/gauss_init.py) on the GPU, beside the same rules in numpy on one CPU thread.

    python tools/time_gauss_init.py [--iters 50] [--warmup 10] [--host-iters 5] [--out DIR] [--name N]
        -> DIR/N.json (default profiles/gauss_init_timing.json)

The mesh is the ellipsoid of tools/time_mesh_labels.py padded to F = 20 908 faces (SMPL-X's count; the padding has no area and is
never chosen); n = 35 000 and 50 000 samples, the two cage sizes of the shipped configurations.  Figures, per n:
  sample_surface   the Python call with the uniforms given and the outputs preallocated (`out=`): eager_us from device events
                   around the call (its five launches, the scratch allocation and the min / max read-back that validates the face
                   indices), wall_us from the host clock around call + synchronise.
  with_rand        the same with `seed=`: adds torch.rand of (n,3) float64 and the allocation of the outputs.
  inflate          one launch over the vertices (V = 10 504).
  numpy_one_thread tests/gauss_init_ref.py::sample_float_path, the float path trimesh documents (cumsum + searchsorted, then the
                   frames, quaternions and barycentrics in float64) on ONE CPU thread of the same box: host clock, median.
  equal_face_ids   share of samples whose face the integer rule and that float path agree on (they differ by the quantum only).
No threshold is set on any of these numbers: they are recorded, not asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from time_calib import alternate, stats  # noqa: E402
from time_mesh_labels import F_SMPLX, ellipsoid  # noqa: E402

COUNTS = (35000, 50000)


def host_us(fn, iters):
    us = []
    for _ in range(iters + 1):
        t0 = time.perf_counter()
        fn()
        us.append((time.perf_counter() - t0) * 1e6)
    return round(float(np.median(us[1:])), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-iters", type=int, default=5)
    ap.add_argument("--name", default="gauss_init_timing", help="file name of the record, without .json")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    import gauss_init_ref as gr
    from d3ga_amd import library_path
    from d3ga_amd.gauss_init import SurfaceSamples, inflate, sample_surface
    os.makedirs(a.out, exist_ok=True)
    torch.set_num_threads(1)
    verts_np, faces_np = ellipsoid()
    faces_np = np.concatenate([faces_np, np.zeros((F_SMPLX - len(faces_np), 3), np.int32)])
    verts_np = verts_np.astype(np.float64)
    verts, faces = torch.from_numpy(verts_np).cuda(), torch.from_numpy(faces_np).cuda()
    rec = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "host_iters": a.host_iters,
           "library": os.path.basename(library_path()), "F": len(faces_np), "V": len(verts_np), "cpus_allowed": len(os.sched_getaffinity(0)),
           "samples": {}}
    grow = lambda: inflate(verts, faces, 0.03)
    rec["inflate"] = {"eager_us": stats(alternate({"hip": grow}, a.iters, a.warmup)["hip"]),
                      "note": "builds the vertex -> face lists on the host on every call (MeshTopology caches them when one is passed)"}
    for n in COUNTS:
        u_np = np.random.default_rng(n).random((n, 3))
        u = torch.from_numpy(u_np).cuda()
        out = SurfaceSamples.empty(n)
        given = lambda: sample_surface(verts, faces, n, uniforms=u, out=out)
        seeded = lambda: sample_surface(verts, faces, n, seed=7)

        def synced():
            given()
            torch.cuda.synchronize()
        us = alternate({"given": given, "seeded": seeded}, a.iters, a.warmup)
        ours = given()
        ours.check()
        ref = gr.sample_float_path(verts_np, faces_np, u_np)
        r = {"sample_surface": {"eager_us": stats(us["given"]), "wall_us": host_us(synced, a.iters)}, "with_rand": {"eager_us": stats(us["seeded"])},
             "numpy_one_thread": {"median_us": host_us(lambda: gr.sample_float_path(verts_np, faces_np, u_np), a.host_iters)},
             "equal_face_ids": round(float((ours.faces.cpu().numpy() == ref[2]).all(1).mean()), 6),
             "max_point_difference": float(np.abs(ours.points.cpu().numpy() - ref[0]).max())}
        rec["samples"][str(n)] = r
        print(json.dumps({n: r}))
    json.dump(rec, open(os.path.join(a.out, a.name + ".json"), "w"), indent=1)


if __name__ == "__main__":
    main()
