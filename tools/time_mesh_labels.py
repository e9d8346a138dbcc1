"""Part-label transfer (d3ga_amd/mesh_labels.py) on the GPU, beside the bytes it has to move and beside the reference's lines.

    python tools/time_mesh_labels.py [--iters 100] [--warmup 20] [--views 512] [--host-iters 3] [--out DIR] [--name N]
        -> DIR/N.json (default profiles/mesh_labels_timing.json)

The fragments come from `rasterize_meshes` of an ellipsoid of 20 800 faces in a person's proportions; the vote runs with F = 20 908
(SMPL-X's face count: the last 108 faces have zero area and are never drawn).  Figures:
  vote            the two launches of LabelTransfer.add_fragments at 747 x 1022 (W x H), B = 1, and 1920 x 1080, B = 4:
                  eager_us (device events), in_graph_us (a replayed graph whose calls ROTATE over independent pix_to_face / label
                  sets, 768 MB per lap or 96 sets, so the 256 MB Infinity Cache holds little of what a launch reads),
                  in_graph_us_same_buffers; each also with D3GA_LABEL_EVERY_PIXEL (no run suppression).  atomics_sent: the keys
                  launch (a) sends, counted on the host by the rule of csrc/mesh_labels_math.h.  kernel_us: per-kernel device time from torch.profiler ("not
                  measured" where the profiler gives none); mark_hbm_floor_us = 4 B H W bytes over 8 TB/s, mark_roofline_share =
                  that over label_mark's kernel time.
  transfer        a Segmenter.run-sized accumulation: --views calls of LabelTransfer.add (rasterize_meshes + vote) at 747 x 1022,
                  B = 1, over 8 cameras around the mesh, then labels(): host clock around the loop, ending in a synchronise.
  grow10          10 rings of grow_mask_region on the device (eager_us, in_graph_us).
  stand_in        what stands in for the reference's lines on this box, written here from the rules: one view's index-put scatter
                  in torch on the GPU (boolean-mask indexing first; host clock, synchronised), and on ONE CPU thread the read-back of
                  the (F, 3 views) label array plus one Python loop over the faces per stage -- np.unique per face for the vote,
                  np.median per face for the filter, set membership per face and ring for the growth -- the per-face library calls
                  the reference's loops make.  The reference's own text is not run here.
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
from time_calib import alternate, graph_time, stats  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
ROTATE_BYTES = 3 * 256 * 2 ** 20
F_SMPLX = 20908
CASES = [(747, 1022, 1), (1920, 1080, 4)]                    # (W, H, B)
EVERY_PIXEL = 1


def ellipsoid(nu=104, nv=100):
    """(verts (V,3) float32, faces (F,3) int32), F = 2 nu nv: rings of a 0.45 x 0.9 x 0.3 ellipsoid, open at the poles"""
    theta = np.linspace(0.05, np.pi - 0.05, nv + 1)[:, None]
    phi = (np.arange(nu) * (2 * np.pi / nu))[None, :]
    x = np.stack([0.45 * np.sin(theta) * np.cos(phi), 0.9 * np.cos(theta) * np.ones_like(phi), 0.3 * np.sin(theta) * np.sin(phi)], -1)
    idx = np.arange((nv + 1) * nu).reshape(nv + 1, nu)
    a, b, c, d = idx[:-1], np.roll(idx, -1, 1)[:-1], idx[1:], np.roll(idx, -1, 1)[1:]
    faces = np.concatenate([np.stack([a, c, b], -1).reshape(-1, 3), np.stack([b, c, d], -1).reshape(-1, 3)])
    return x.reshape(-1, 3).astype(np.float32), faces.astype(np.int32)


def look_at(eye):
    eye = np.asarray(eye, np.float64)
    fwd = -eye / np.linalg.norm(eye)
    right = np.cross([0.0, -1.0, 0.0], fwd)
    right /= np.linalg.norm(right)
    R = np.stack([right, np.cross(fwd, right), fwd])
    return R, -R @ eye


def cameras_around(n, H, W, B):
    """n batches of B cameras on a circle around the mesh, the 1.8-high ellipsoid filling 85 % of the frame's height"""
    from d3ga_amd.mesh_render import MeshCameras
    dist, out = 3.0, []
    f = 0.85 * H * dist / 1.8
    K = np.array([[f, 0, 0.5 * W], [0, f, 0.5 * H], [0, 0, 1.0]])
    for k in range(n):
        Rs, ts = zip(*[look_at([dist * np.sin(a), 0.3, dist * np.cos(a)]) for a in 2 * np.pi * (k + np.arange(B) / B) / n])
        out.append(MeshCameras(np.stack(Rs), np.stack(ts), K, (H, W)))
    return out


def atomics_sent(p2f, F, suppress):
    """the keys launch (a) sends, by ml_sends: a pixel is silent when its right neighbour in the same wavefront shows its face"""
    ok = (p2f >= 0) & (p2f < F)
    if not suppress:
        return int(ok.sum())
    W = p2f.shape[-1]
    same = np.zeros_like(ok)
    same[..., :-1] = p2f[..., :-1] == p2f[..., 1:]
    same[..., np.arange(W) % 64 == 63] = False
    return int((ok & ~same).sum())


def kernel_times(call, n=20):
    """name -> mean device us per launch of this library's label kernels, from torch.profiler; {} if it reports none"""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(n):
                call()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            if "label_" in e.key and "kernel" in e.key:
                total = getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0)
                if total and e.count:
                    out[e.key.split("(")[0].split("::")[-1]] = round(total / e.count, 2)
        return out
    except Exception as exc:                                  # the record says so instead of guessing
        return {"error": f"{type(exc).__name__}: {exc}"[:200]}


# ---- stand-ins for the reference's host work, written here from the rules of DESIGN.md 4.4r: one Python loop over the faces per
# stage with the same library call per face (np.unique, np.median, set membership) -------------------------------------------------
def rings_of(table):
    """face -> list of its neighbours, from the (F,3) table"""
    return {f: [int(n) for n in row if n >= 0] for f, row in enumerate(table.tolist())}


def loop_majority(part):
    """(F, n) labels, 0 = no vote -> (F,): np.unique per row"""
    out = np.zeros(len(part), np.int64)
    for f, row in enumerate(part):
        voted = row[row > 0]
        if voted.size:
            values, counts = np.unique(voted, return_counts=True)
            out[f] = values[np.argmax(counts)]
    return out


def loop_median(rings, labels):
    return np.array([int(np.median(labels[rings[f]])) for f in range(len(rings))])


def loop_growth(rings, mask, n_rings):
    mask = np.array(mask, bool)
    for _ in range(n_rings):
        inside = set(np.flatnonzero(mask).tolist())
        marked = set()
        for f in range(len(rings)):
            hits = sum(n in inside for n in rings[f])
            if 0 < hits < len(rings[f]):
                marked.update(rings[f])
        mask[list(marked)] = True
    return mask


def torch_scatter(pix_to_face, image, n_face):
    """One view's labels onto the faces with torch's index-put, duplicates and all: pix_to_face, image (H,W) -> (F,) int64"""
    hit = pix_to_face >= 0
    out = torch.zeros(n_face, dtype=torch.int64, device=pix_to_face.device)
    out[pix_to_face[hit].long()] += image[hit].long()
    return out


def host_ms(fn, iters):
    ms = []
    for _ in range(iters + 1):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ms[1:])), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--views", type=int, default=512)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--name", default="mesh_labels_timing", help="file name of the record, without .json")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    from d3ga_amd import library_path
    from d3ga_amd.mesh_labels import LabelTransfer, grow_mask_region
    from d3ga_amd.mesh_render import rasterize_meshes
    os.makedirs(a.out, exist_ok=True)
    torch.set_num_threads(1)
    verts_np, faces_np = ellipsoid()
    faces_np = np.concatenate([faces_np, np.zeros((F_SMPLX - len(faces_np), 3), np.int32)])     # 108 faces of zero area: never drawn
    F, L = len(faces_np), 5
    gt = (1 + (np.arange(F) // (F // 4 + 1))).astype(np.int32)
    t_gt = torch.from_numpy(gt).cuda()
    verts = torch.from_numpy(verts_np).cuda()
    rec = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "library": os.path.basename(library_path()), "F": F,
           "n_labels": L, "rotate_bytes": ROTATE_BYTES, "hbm_bytes_per_s": HBM_BYTES_PER_S, "cpus_allowed": len(os.sched_getaffinity(0)), "vote": {}}

    def paint(p2f):
        return torch.where(p2f >= 0, t_gt[p2f.clamp(min=0).long()], torch.zeros_like(p2f))[:, None].contiguous()

    for W, H, B in CASES:
        cams = cameras_around(8, H, W, B)
        vb = verts[None].expand(B, -1, -1).contiguous()
        frags = [rasterize_meshes(c, vb, faces_np).pix_to_face.clone() for c in cams]
        parts = [paint(p) for p in frags]
        p2f_host = frags[0].cpu().numpy()
        lt = LabelTransfer(faces_np, L, B, H, W, n_verts=len(verts_np))
        nbytes = 4 * B * H * W
        r = {"size": [W, H], "B": B, "covered_pixels": int((p2f_host >= 0).sum()),
             "faces_seen": int(len(np.unique(p2f_host[p2f_host >= 0]))), "mark_bytes": nbytes, "mark_hbm_floor_us": round(nbytes / HBM_BYTES_PER_S * 1e6, 3)}
        variants = {"default": 0, "every_pixel": EVERY_PIXEL}
        sets = int(min(96, max(2, -(-ROTATE_BYTES // (2 * nbytes)))))
        pool = [(frags[k % 8].clone(), parts[k % 8].clone()) for k in range(sets)]
        for name, flags in variants.items():
            lt._flags = flags
            lt.reset()
            turn = [0]

            def same():
                lt.add_fragments(frags[0], parts[0])

            def rotate():
                lt.add_fragments(*pool[turn[0] % sets])
                turn[0] += 1
            v = {"eager_us": stats(alternate({"hip": same}, a.iters, a.warmup)["hip"]),
                 "in_graph_us": round(graph_time(rotate, calls=sets * max(1, -(-20 // sets))), 2), "in_graph_sets": sets,
                 "in_graph_us_same_buffers": round(graph_time(same), 2),
                 "atomics_sent": atomics_sent(p2f_host, F, not flags & EVERY_PIXEL), "kernel_us": kernel_times(same) or "not measured"}
            mark = [t for k, t in v["kernel_us"].items() if "label_mark" in k] if isinstance(v["kernel_us"], dict) else []
            v["mark_roofline_share"] = round(r["mark_hbm_floor_us"] / mark[0], 3) if mark else "not measured"
            v["both_launches_roofline_share"] = round(r["mark_hbm_floor_us"] / v["in_graph_us"], 3)
            lt.check()
            r[name] = v
            print(json.dumps({name: v}))
        lt._flags = 0
        # the index-put scatter on the same fragments, view 0 of the batch, on the GPU
        torch.cuda.synchronize()

        def scatter():
            torch_scatter(frags[0][0], parts[0][0, 0], F)
            torch.cuda.synchronize()
        r["torch_scatter_gpu_ms_per_view"] = host_ms(scatter, 20)
        rec["vote"][f"{W}x{H}_B{B}"] = r
        if (W, H, B) == CASES[0]:
            # ---- a Segmenter.run-sized transfer ------------------------------------------------------------------------------
            lt.reset()
            for k in range(8):
                lt.add(cams[k], vb, parts[k])
            lt.labels()
            lt.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(a.views):
                lt.add(cams[k % 8], vb, parts[k % 8])
            labels = lt.labels()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            lt.check()
            hist = lt.counts().cpu().numpy()
            got = lt.labels(median=False).cpu().numpy()
            seen = hist.sum(1) > 0
            rec["transfer"] = {"views": a.views, "size": [W, H], "B": B, "total_ms": round(ms, 2), "ms_per_view": round(ms / a.views, 4),
                               "faces_seen": int(seen.sum()), "labels_equal_truth_on_seen_faces": bool((got[seen] == gt[seen]).all())}
            print(json.dumps(rec["transfer"]))
            # ---- growth ------------------------------------------------------------------------------------------------------
            table = lt.neighbours
            mask = torch.from_numpy(gt == 2).cuda()
            grow = lambda: grow_mask_region(table, mask, 10)
            rec["grow10"] = {"F": F, "eager_us": stats(alternate({"hip": grow}, a.iters, a.warmup)["hip"]), "in_graph_us": round(graph_time(grow), 2),
                             "note": "the Python call allocates its output and scratch and converts bool <-> uint8 around the 10 launches"}
            print(json.dumps(rec["grow10"]))
            # ---- the stand-in host loops, one CPU thread -------------------------------------------------------------------------
            table_np = table.cpu().numpy()
            n_ref = int(np.flatnonzero((table_np >= 0).any(1)).max()) + 1          # the faces with neighbours: the ellipsoid's
            assert (table_np[:n_ref] >= 0).any(1).all() and table_np[:n_ref].max() < n_ref
            rings = rings_of(table_np[:n_ref])
            views = [torch_scatter(frags[k][0], parts[k][0, 0], F) for k in range(8)]
            part_dev = torch.stack([views[k % 8] for k in range(a.views)], 1).repeat_interleave(3, dim=1).int()    # three equal columns per view
            t0 = time.perf_counter()
            part_host = part_dev.cpu().numpy()
            readback_ms = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            voted = loop_majority(part_host[:n_ref])
            vote_ms = (time.perf_counter() - t0) * 1e3
            median_ms = host_ms(lambda: loop_median(rings, voted), a.host_iters)
            mask_np = (gt == 2)[:n_ref]
            grow_ms = host_ms(lambda: loop_growth(rings, mask_np, 10), a.host_iters)
            ours_grown = grow_mask_region(table, mask, 10).cpu().numpy()[:n_ref]
            rec["stand_in_host_one_thread"] = {"faces": n_ref, "columns": int(part_host.shape[1]), "readback_ms": round(readback_ms, 2),
                                               "majority_loop_ms": round(vote_ms, 2), "median_loop_ms": median_ms, "growth_loop_10_rings_ms": grow_ms,
                                               "labels_equal_ours": bool(np.array_equal(labels.cpu().numpy()[:n_ref], loop_median(rings, voted))),
                                               "grown_equal_ours": bool(np.array_equal(ours_grown, loop_growth(rings, mask_np, 10)))}
            print(json.dumps(rec["stand_in_host_one_thread"]))
        del pool, lt
        torch.cuda.empty_cache()
    json.dump(rec, open(os.path.join(a.out, a.name + ".json"), "w"), indent=1)


if __name__ == "__main__":
    main()
