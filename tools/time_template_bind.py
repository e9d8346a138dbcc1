"""Template binding (d3ga_amd/template_bind.py) on the GPU, beside the oracle's numpy form on one CPU thread.

    python tools/time_template_bind.py [--iters 20] [--warmup 3] [--host-iters 2] [--out DIR] [--name N]
        -> DIR/N.json (default profiles/template_bind_timing.json)

The shape is SMPL-X's: V = 10 475 vertices, F = 20 908 faces (a tube of 419 rings of 25 vertices with eight ears on one rim), a
55-column skinning table (a synthetic model of `d3ga_amd.synthetic`), and a cage of 24 000 vertices.  Figures, median per call:
  loop_plan            keys, torch.sort, the plan kernels and the one read-back                        (host clock: it synchronises)
  loop_subdivide       positions and the (V, 55) table over a given plan, plus the faces                (device events)
  nearest_dense        every dense vertex against the 10 475 template vertices                          (device events)
  unpose_dense         the dense vertices, dense table                                                  (device events)
  nearest_cage         24 000 cage vertices against the inflated template (normals + search)            (device events)
  unpose_cage          24 000 cage vertices                                                             (device events)
  bind_body_template   the whole call, star pose included                                               (host clock)
  bind_cage            the whole call                                                                   (host clock)
  numpy_one_thread     tests/template_bind_ref.py: plan + stencils + faces, nearest (float32 distances, chunked), unpose -- host clock.
No threshold is set on any of these numbers: they are recorded, not asserted."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from time_calib import alternate, stats  # noqa: E402

RINGS, RING, EARS, N_CAGE = 419, 25, 8, 24000


def tube():
    """(verts (10475,3) float32, faces (20908,3) int32)"""
    t = np.linspace(0.03, np.pi - 0.03, RINGS)[:, None]
    phi = (np.arange(RING) * (2 * np.pi / RING))[None, :]
    x = np.stack([0.45 * np.sin(t) * np.cos(phi), 0.9 * np.cos(t) * np.ones_like(phi), 0.3 * np.sin(t) * np.sin(phi)], -1)
    idx = np.arange(RINGS * RING).reshape(RINGS, RING)
    a, b, c, d = idx[:-1], np.roll(idx, -1, 1)[:-1], idx[1:], np.roll(idx, -1, 1)[1:]
    ears = np.array([[2 * i, 2 * i + 1, 2 * i + 2] for i in range(EARS)])
    faces = np.concatenate([np.stack([a, c, b], -1).reshape(-1, 3), np.stack([b, c, d], -1).reshape(-1, 3), ears])
    return x.reshape(-1, 3).astype(np.float32), faces.astype(np.int32)


def host_us(fn, iters):
    us = []
    for _ in range(iters + 1):
        t0 = time.perf_counter()
        fn()
        us.append((time.perf_counter() - t0) * 1e6)
    return round(float(np.median(us[1:])), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-iters", type=int, default=2)
    ap.add_argument("--name", default="template_bind_timing", help="file name of the record, without .json")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    import template_bind_ref as tr
    import d3ga_amd.synthetic as syn
    from d3ga_amd import library_path
    from d3ga_amd.body_model import SMPLlayer
    from d3ga_amd.template_bind import bind_body_template, bind_cage, loop_plan, loop_subdivide, nearest_vertex, star_pose, unpose
    os.makedirs(a.out, exist_ok=True)
    torch.set_num_threads(1)
    verts_np, faces_np = tube()
    V, F = len(verts_np), len(faces_np)
    assert (V, F) == (10475, 20908)
    data = syn.smpl_model_data("smplx", seed=5, V=V)
    data["f"], data["v_template"] = faces_np.astype(np.int64), verts_np.astype(np.float64)
    with tempfile.TemporaryDirectory() as d:
        syn.write_smpl_model(os.path.join(d, "SMPLX_NEUTRAL.npz"), data)
        layer = SMPLlayer(d, model_type="smplx", gender="neutral").cuda()
    star, _, A, bs = star_pose(layer)
    v, f, w = star[0].contiguous(), layer.faces_tensor, layer.weights
    plan = loop_plan(f, V).check()
    nv, nf, nw = loop_subdivide(v, f, w, plan=plan)
    ids = nearest_vertex(v, f, nv)
    rng = np.random.default_rng(3)
    cage = torch.from_numpy((verts_np[rng.integers(0, V, N_CAGE)] * 1.08 + rng.normal(size=(N_CAGE, 3)) * 0.005).astype(np.float32)).cuda()
    cage_ids = nearest_vertex(v, f, cage, 0.01)
    binding = bind_body_template(layer)

    def synced(fn):
        def run():
            fn()
            torch.cuda.synchronize()
        return run
    dev = alternate({"loop_subdivide": lambda: loop_subdivide(v, f, w, plan=plan), "nearest_dense": lambda: nearest_vertex(v, f, nv),
                     "unpose_dense": lambda: unpose(nv, A[0], nw, ids, bs[0]), "nearest_cage": lambda: nearest_vertex(v, f, cage, 0.01),
                     "unpose_cage": lambda: unpose(cage, A[0], nw, cage_ids, bs[0])}, a.iters, a.warmup)
    rec = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "host_iters": a.host_iters,
           "library": os.path.basename(library_path()), "V": V, "F": F, "E": plan.E, "columns": int(w.shape[1]), "dense_vertices": int(nv.shape[0]),
           "cage_vertices": N_CAGE, "max_valence": plan.max_valence, "cpus_allowed": len(os.sched_getaffinity(0)),
           "gpu": {k: {"eager_us": stats(us)} for k, us in dev.items()}}
    rec["gpu"]["loop_plan"] = {"wall_us": host_us(synced(lambda: loop_plan(f, V)), a.iters)}
    rec["gpu"]["bind_body_template"] = {"wall_us": host_us(synced(lambda: bind_body_template(layer)), a.iters)}
    rec["gpu"]["bind_cage"] = {"wall_us": host_us(synced(lambda: bind_cage(layer, binding, cage, 0.01)), a.iters)}
    print(json.dumps(rec["gpu"]))
    # the oracle's numpy form, one thread
    vh, fh, wh = v.cpu().numpy(), f.cpu().numpy(), w.cpu().numpy()
    Ah, bsh, nvh, nwh, idh = A[0].cpu().numpy(), bs[0].cpu().numpy(), nv.cpu().numpy(), nw.cpu().numpy(), ids.cpu().numpy()

    def subdivide():
        p = tr.plan(fh, V)
        return tr.stencil(p, vh), tr.stencil(p, wh), tr.new_faces(p)
    t0 = time.perf_counter()
    near = tr.nearest(vh, nvh)                               # seconds per call: timed once
    near_us = round((time.perf_counter() - t0) * 1e6, 1)
    rec["numpy_one_thread"] = {"plan_and_subdivide": {"median_us": host_us(subdivide, a.host_iters)},
                               "nearest_dense": {"once_us": near_us},
                               "unpose_dense": {"median_us": host_us(lambda: tr.unpose(nvh, Ah, nwh, idh, bsh), a.host_iters)}}
    got = subdivide()
    rec["equal_to_numpy"] = {"vertices": bool(tr.same_bits(got[0], nvh)), "weights": bool(tr.same_bits(got[1], nwh)),
                             "faces": bool(np.array_equal(got[2], nf.cpu().numpy())), "nearest": bool(np.array_equal(near, idh))}
    print(json.dumps({k: rec[k] for k in ("numpy_one_thread", "equal_to_numpy")}))
    json.dump(rec, open(os.path.join(a.out, a.name + ".json"), "w"), indent=1)


if __name__ == "__main__":
    main()
