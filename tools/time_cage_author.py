"""Cage surface authoring (d3ga_amd/cage_author.py) on the GPU, beside the oracle's numpy / scipy form on the same box.

    python tools/time_cage_author.py [--iters 5] [--warmup 1] [--radii 120,60] [--no-oracle] [--out DIR] [--name N]
        -> DIR/N.json (default profiles/cage_author_timing.json)

The mesh is a closed body-sized figure of capsule limbs with about 20 000 faces (tests/cage_author_ref.py::capsule_figure cut from a
61^3 grid).  Per radius, median wall time per call with a device synchronisation on either side (every stage reads something back,
so the host clock is the honest one): prepare, voxelize (surface only), fill_holes (+ its number of rounds), isosurface,
loop_plan of the surface, smooth_improved x25 and smooth_taubin x10 over that plan, keep_components, and the whole cage_processor,
eager.  Then the oracle (tests/cage_author_ref.py: numpy SAT, scipy binary_fill_holes, the Python marching-tetrahedra loop, scipy.sparse
smoothers, csgraph components), once per stage: plain numpy / scipy code paths that run on one CPU thread.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def wall_us(fn, iters, warmup):
    us, out = [], None
    for i in range(warmup + iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if i >= warmup:
            us.append((time.perf_counter() - t0) * 1e6)
    return {"median_us": round(float(np.median(us)), 1), "min_us": round(float(np.min(us)), 1), "max_us": round(float(np.max(us)), 1)}, out


def once_us(fn):
    t0 = time.perf_counter()
    out = fn()
    return round((time.perf_counter() - t0) * 1e6, 1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--radii", default="120,60")
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--name", default="cage_author_timing")
    a = ap.parse_args()
    import cage_author_ref as cr
    import d3ga_amd as d
    v, f = cr.capsule_figure(r=30, through_host_build=True)
    tv, tf = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "V": len(v), "F": len(f),
           "cpus_allowed": len(os.sched_getaffinity(0)), "radius": {}}
    for radius in (int(r) for r in a.radii.split(",")):
        g = {}
        g["prepare"], (pv, centre) = wall_us(lambda: d.prepare(tv, tf, 0.01, 0.8), a.iters, a.warmup)
        g["voxelize_surface"], surf = wall_us(lambda: d.voxelize(pv, tf, radius, fill=False), a.iters, a.warmup)
        g["fill_holes"], filled = wall_us(lambda: d.fill_holes(surf), a.iters, a.warmup)
        g["fill_holes"]["rounds"] = filled.rounds
        g["isosurface"], (iv, jf) = wall_us(lambda: d.isosurface(filled, centre, (0.8, 0.8, 1.0)), a.iters, a.warmup)
        g["loop_plan"], plan = wall_us(lambda: d.loop_plan(jf, len(iv)), a.iters, a.warmup)
        g["smooth_improved_x25"], sm = wall_us(lambda: d.smooth_improved(iv, jf, 25, 0.25, plan=plan).check(), a.iters, a.warmup)
        g["smooth_taubin_x10"], tb = wall_us(lambda: d.smooth_taubin(sm.vertices, jf, 10, plan=plan).check(), a.iters, a.warmup)
        g["keep_components"], _ = wall_us(lambda: d.keep_components(tb.vertices, jf, 70, plan=plan), a.iters, a.warmup)
        g["cage_processor"], (cv, cf) = wall_us(lambda: d.cage_processor(tv, tf, 0, radius, 0.01), a.iters, a.warmup)
        entry = {"gpu": g, "surface_voxels": int(surf.dense().sum()), "filled_voxels": int(filled.dense().sum()), "vertices": len(iv), "faces": len(jf),
                 "cage_vertices": cv.shape[1], "cage_faces": cf.shape[1]}
        if not a.no_oracle:
            o = {}
            hp = pv.cpu().numpy()
            o["voxelize_surface_us"], s = once_us(lambda: cr.surface(hp, f, radius))
            o["fill_holes_us"], fl = once_us(lambda: cr.fill(s))
            o["isosurface_us"], (ov, of, _) = once_us(lambda: cr.isosurface(fl, centre.cpu().numpy(), (0.8, 0.8, 1.0)))
            o["smooth_improved_x25_us"], os_ = once_us(lambda: cr.smooth_improved(ov, of, 25, 0.25))
            o["smooth_taubin_x10_us"], ot = once_us(lambda: cr.smooth_taubin(os_, of, 10))
            o["keep_components_us"], _ = once_us(lambda: cr.keep_components(ot, of, 70))
            o["sum_us"] = round(sum(o.values()), 1)
            entry["numpy_scipy"] = o
            entry["equal_to_numpy"] = {"surface": bool(np.array_equal(s, surf.dense().cpu().numpy())), "filled": bool(np.array_equal(fl, filled.dense().cpu().numpy())),
                                       "faces": bool(np.array_equal(of, jf.cpu().numpy())), "vertices": bool(np.array_equal(ov, iv.cpu().numpy()))}
        res["radius"][str(radius)] = entry
        print(radius, json.dumps(entry), flush=True)
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, a.name + ".json")
    with open(path, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
