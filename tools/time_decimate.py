"""Quadric edge-collapse decimation (d3ga_amd/cage_author.py::decimate) on the GPU, beside the g++ build of csrc/decimate_math.h on one
CPU thread of the same box.

    python tools/time_decimate.py [--iters 5] [--warmup 1] [--cases 120:15000,120:10000,60:10000] [--no-host] [--out DIR] [--name N]
        -> DIR/N.json (default profiles/decimate_timing.json)
    python tools/time_decimate.py --trace-only [--cases ...]          the decimations alone, twice each: the program of a
        `rocprofv3 --kernel-trace --stats` run of its own (no counters in that run)
    python tools/time_decimate.py --merge-stats STATS.csv             adds that run's per-kernel rows to the JSON

The mesh is the closed 19 700-face figure of tools/time_cage_author.py.  Per case radius:target, median wall time per call with a
device synchronisation on either side (every round reads two counts and the plan's sizes back, so the host clock is the honest
one): `decimate` of the Taubin-filtered isosurface with its number of rounds, and the share of it that `loop_plan` plus the vertex ->
face lists take (timed on the first round's mesh, times the rounds: an upper estimate, later rounds are smaller); then the
whole `cage_processor(..., decimation="quadric")` next to the undecimated `cage_processor` of the same run.  Then the g++ build, once,
and whether the kernels gave its bits.  No threshold is set on any of these numbers: they are recorded, not asserted."""
import argparse
import csv
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


def surface(d, tv, tf, radius):
    """the Taubin-filtered isosurface `simplify` hands to `decimate`"""
    cv, cf = d.create_cage(tv, tf, radius, 0.01)
    sv, sf = d.smooth_cage(cv, cf)
    return d.smooth_taubin(sv, sf, iterations=10).check().vertices, sf


def merge_stats(path, stats_csv):
    res = json.load(open(path))
    rows = [r for r in csv.DictReader(open(stats_csv))]
    rows.sort(key=lambda r: -float(r["TotalDurationNs"]))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    res["kernel_stats"] = {"source": "rocprofv3 --kernel-trace --stats of `tools/time_decimate.py --trace-only`, a run of its own; every kernel of the process",
                           "total_ms": round(total / 1e6, 3),
                           "kernels": [{"name": r["Name"][:96], "calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 2),
                                        "total_ms": round(float(r["TotalDurationNs"]) / 1e6, 3)} for r in rows[:24]]}
    with open(path, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("merged", stats_csv, "into", path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cases", default="120:15000,120:10000,60:10000")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--merge-stats")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--name", default="decimate_timing")
    a = ap.parse_args()
    path = os.path.join(a.out, a.name + ".json")
    if a.merge_stats:
        return merge_stats(path, a.merge_stats)
    import cage_author_ref as cr
    import d3ga_amd as d
    from d3ga_amd.cage_author import _vertex_faces
    if not torch.cuda.is_available():
        raise SystemExit("time_decimate: no GPU; these numbers are taken on the device or not at all")
    cases = [tuple(int(x) for x in c.split(":")) for c in a.cases.split(",")]
    v, f = cr.capsule_figure(r=30, through_host_build=True)
    tv, tf = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    if a.trace_only:
        for radius, target in cases:
            sv, sf = surface(d, tv, tf, radius)
            for _ in range(2):
                out = d.decimate(sv, sf, tris_target=target).check()
            torch.cuda.synchronize()
            print(radius, target, out.faces.shape[0], out.rounds, flush=True)
        return
    import decimate_ref as dr
    res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "V": len(v), "F": len(f),
           "cpus_allowed": len(os.sched_getaffinity(0)), "case": {}}
    plain = {}
    for radius, target in cases:
        sv, sf = surface(d, tv, tf, radius)
        g = {}
        g["decimate"], out = wall_us(lambda: d.decimate(sv, sf, tris_target=target).check(), a.iters, a.warmup)
        g["decimate"]["rounds"] = out.rounds

        def connectivity():
            return _vertex_faces(d.loop_plan(sf, sv.shape[0]))
        g["loop_plan_and_vertex_faces_first_round"], _ = wall_us(connectivity, a.iters, a.warmup)
        g["cage_processor_quadric"], (cv, cf) = wall_us(lambda: d.cage_processor(tv, tf, target, radius, 0.01, decimation="quadric"), a.iters, a.warmup)
        if radius not in plain:
            plain[radius], _ = wall_us(lambda: d.cage_processor(tv, tf, 0, radius, 0.01), a.iters, a.warmup)
        g["cage_processor_undecimated"] = plain[radius]
        entry = {"gpu": g, "faces_in": sf.shape[0], "vertices_in": sv.shape[0], "faces_out": out.faces.shape[0], "vertices_out": out.vertices.shape[0],
                 "cage_faces": cf.shape[1]}
        if not a.no_host:
            hv, hf = sv.cpu().numpy(), sf.cpu().numpy()
            t0 = time.perf_counter()
            want = dr.host_decimate(hv, hf, target)
            entry["host_build_one_thread_us"] = round((time.perf_counter() - t0) * 1e6, 1)
            entry["equal_to_host_build"] = bool(np.array_equal(want[1], out.faces.cpu().numpy()) and cr.same_bits(want[0], out.vertices.cpu().numpy())
                                                and want[2] == out.rounds)
        res["case"][f"{radius}:{target}"] = entry
        print(radius, target, json.dumps(entry), flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(path, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
