"""`knn_points(p, p, K=4)` (d3ga_amd/knn.py, csrc/knn.hip) with both methods at the actor02 size, 135 000 points, and at 500 000
points, next to `knn_mean_dist2` on the same points (the nearest existing yardstick: the same search without indices, three
distances kept) and next to a chunked `torch.cdist` + `topk`.

    python tools/time_knn.py [--reps 5] [--out DIR]      -> DIR/knn_P<P>.json (default profiles/)

The points fill a standing ellipsoid (tools/time_point_render.py's body cloud).  Three kinds of figures, all medians of device
events around eager calls:
    call_ms      the Python call as a user makes it: for the grid method this includes the host read of the bounding box and the
                 CSR built with torch ops (sort, bincount, cumsum)
    kernel_ms    the entry point alone on a prepared grid (d3ga_knn_points_grid / d3ga_knn3_mean_dist2_grid), or the exhaustive
                 entry point
    cdist_topk   torch.cdist(...)**2 and topk(4, largest=False) over chunks of 2048 queries, timed on the first 16384 queries and
                 scaled to P (it is linear in the number of chunks); it orders by a distance that went through a square root
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
SIZES = (135000, 500000)


def event_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return round(float(np.median(out)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    from time_point_render import body_cloud
    from d3ga_amd import _lib, knn_points
    from d3ga_amd.knn import _grid
    from d3ga_amd.tetra import knn_mean_dist2
    os.makedirs(a.out, exist_ok=True)
    L, p = _lib.lib(), lambda t: ctypes.c_void_p(t.data_ptr())
    for P in SIZES:
        pts = torch.from_numpy(body_cloud(P)).cuda()
        both = pts[None]
        call = {"knn_points_grid": event_ms(lambda: knn_points(both, both, K=4, method="grid"), a.reps),
                "knn_points_exhaustive": event_ms(lambda: knn_points(both, both, K=4, method="exhaustive"), max(2, a.reps // 2)),
                "knn_mean_dist2_grid": event_ms(lambda: knn_mean_dist2(pts), a.reps),
                "knn_mean_dist2_exhaustive": event_ms(lambda: knn_mean_dist2(pts, method="exhaustive"), max(2, a.reps // 2))}
        start, items, origin_h, dims = _grid(pts)
        dists, idx = torch.empty(P, 4, device="cuda"), torch.empty(P, 4, dtype=torch.int64, device="cuda")
        mean = torch.empty(P, device="cuda")
        s = _lib.stream_handle
        kernel = {"d3ga_knn_points_grid": event_ms(lambda: _lib.check(L.d3ga_knn_points_grid(P, P, 4, p(pts), p(pts), p(start), p(items), origin_h, dims,
                                                                                          p(dists), p(idx), s()), "grid"), a.reps),
                  "d3ga_knn3_mean_dist2_grid": event_ms(lambda: _lib.check(L.d3ga_knn3_mean_dist2_grid(P, p(pts), p(start), p(items), origin_h, dims,
                                                                                                    p(mean), s()), "knn3 grid"), a.reps)}
        g, e = knn_points(both, both, K=4, method="grid"), knn_points(both, both, K=4, method="exhaustive")
        same = bool(torch.equal(g.idx, e.idx) and torch.equal(g.dists.view(torch.int32), e.dists.view(torch.int32)))
        rel = float(((g.dists[0, :, 1:].mean(-1) - knn_mean_dist2(pts)).abs() / knn_mean_dist2(pts)).max())
        n_q, chunk = 16384, 2048

        def cdist_topk():
            for c in range(0, n_q, chunk):
                d2 = torch.cdist(pts[c:c + chunk], pts) ** 2
                d2.topk(4, dim=1, largest=False)

        sub = event_ms(cdist_topk, max(2, a.reps // 2))
        rec = {"points": P, "K": 4, "device": torch.cuda.get_device_name(0), "grid_dims": list(dims), "cell_edge": origin_h[3],
               "call_ms": call, "kernel_ms": kernel, "grid_equals_exhaustive_bitwise": same, "mean_of_3_vs_knn_mean_dist2_max_rel": rel,
               "cdist_topk_ms": round(sub * P / n_q, 1), "cdist_topk_note": f"timed on {n_q} queries in chunks of {chunk}, scaled linearly to {P}"}
        print(f"P={P}: {json.dumps(rec)}")
        json.dump(rec, open(os.path.join(a.out, f"knn_P{P}.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
