#!/usr/bin/env python3
"""Bit-for-bit comparison of what the preprocess kernels leave, between two builds of the library -- what tools/fwd_bits_ab.py
does not reach: radii, tile offsets and sorted lists, counters, and the full parameter gradients of a backward.

    D3GA_LIB_PATH=tools/_build/libd3ga_hip_parent.so python tools/pre_bits_ab.py digest bits_parent.json
    python tools/pre_bits_ab.py digest bits_new.json
    python tools/pre_bits_ab.py compare bits_parent.json bits_new.json      # exit 1 on any differing digest

Inputs: the cases of tests/test_gpu_per_gaussian_loads.py (64 x 48, P in {1, 65, 209, 257}; training forward, forward only,
precomputed colours; index offset 17; wavefront 1 culled; the one-tile raster; covariances from scale and rotation in three layouts;
the windowed camera slot; k = 2, 3, 4 views) and camera 0 of C3.  The backward is driven by a FIXED, SPARSE dL/dimage:
one pixel per 16 x 16 tile (per 128 x 128 pixels at C3), so that almost every Gaussian receives contributions from one pixel only and the float atomics have no
sum to reorder; dL/dmeans3D then pins the direction Jacobian the forward left (dcol)."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def one_case(g, inp, use_sh, train, from_sr=False):
    import torch
    from d3ga_amd import rasterizer as R
    import test_gpu_per_gaussian_loads as T
    dev = "cuda"
    bg = torch.tensor([0.2, 0.4, 0.6])
    rast = R.GaussianRasterizer(T._settings(inp, bg, 3 if use_sh else 0))
    leaf = lambda k: g[k].to(dev).clone().contiguous().requires_grad_(train)
    means, op = leaf("means3D"), leaf("opacities")
    geo = (leaf("scales"), leaf("rots")) if from_sr else (leaf("cov6"),)
    col = leaf("shs") if use_sh else leaf("rgb")
    with torch.set_grad_enabled(train):
        color, radii, _ = rast(means3D=means, means2D=None, opacities=op, shs=col if use_sh else None,
                               colors_precomp=None if use_sh else col,
                               **(dict(scales=geo[0], rotations=geo[1]) if from_sr else dict(cov3D_precomp=geo[0])))
    start, plist, _ = R.last_tile_lists(inp["W"], inp["H"])
    cnt = R.last_counters()
    out = {"render": sha(color), "radii": sha(radii), "tile_start": sha(start), "point_list": sha(plist),
           "counters": json.dumps({k: (int(v) if not isinstance(v, bool) else v) for k, v in sorted(cnt.items())})}
    if train:
        gpix = torch.zeros_like(color)
        step = 16 if inp["W"] <= 64 else 128            # one pixel per tile; C3: one per 8 x 8 tiles, its splats are a few pixels wide
        gpix[:, 5::step, 9::step] = torch.tensor([0.75, -0.5, 0.25], device=dev).view(3, 1, 1)
        (color * gpix).sum().backward()
        out.update({"d_means3D": sha(means.grad), "d_opacity": sha(op.grad), "d_colour": sha(col.grad)})
        out.update({"d_geo%d" % k: sha(t.grad) for k, t in enumerate(geo)})
    return out


def lists_and_counters(W, H, rows=1):
    """what the most recent forward left in its binning buffer (rows: views of a batch, one frame of rows x tile rows)"""
    import torch
    from d3ga_amd import rasterizer as R
    binning, cap = R._last[torch.cuda.current_device()]
    start, plist, _ = R.tile_lists(binning, W, 16 * ((H + 15) // 16) * rows, cap)
    cnt = R.last_counters()
    return {"tile_start": sha(start), "point_list": sha(plist),
            "counters": json.dumps({k: (int(v) if not isinstance(v, bool) else v) for k, v in sorted(cnt.items())})}


def renderer_cases(res):
    """the windowed camera slot (P = 209 behind an off-centre principal point) and k = 2, 3, 4 cameras of one set of Gaussians"""
    import torch
    import test_gpu_per_gaussian_loads as T
    from d3ga_amd import synthetic as syn
    from d3ga_amd.renderer import render, render_views
    dev, P = "cuda", 209
    bg = torch.tensor([0.3, 0.6, 0.1], device=dev)
    for train in (False, True):
        inp = T._scene(T.SEEDS[P], cx=23, cy=31)
        g = T._gaussians(P, inp)
        pkg = {"means3D": g["means3D"].to(dev).requires_grad_(train), "cov3D_precomp": g["cov6"].to(dev), "opacities": g["opacities"].to(dev),
               "shs": g["shs"].to(dev), "rgb": None, "sh_degree": 3}
        with torch.set_grad_enabled(train):
            out = {"render": sha(render(inp["batch"], pkg, bg, crop_window=True)["render"])}
        res["cases"]["P209/windowed/%s" % ("train" if train else "forward_only")] = out
        g = T._gaussians(P)
        pkg.update(means3D=g["means3D"].to(dev).requires_grad_(train), cov3D_precomp=g["cov6"].to(dev), opacities=g["opacities"].to(dev),
                   shs=g["shs"].to(dev))
        for k in (2, 3, 4):
            batches = [syn.make_batch(T.W, T.H, azimuth=0.4 + 0.7 * v) for v in range(k)]
            with torch.set_grad_enabled(train):
                out = {"render": sha(render_views(batches, pkg, bg)["render"])}
            out.update(lists_and_counters(T.W, T.H, k))
            res["cases"]["P209/views%d/%s" % (k, "train" if train else "forward_only")] = out


def digest(out_path):
    import torch
    import test_gpu_per_gaussian_loads as T
    from d3ga_amd import _lib
    from util import scene_inputs
    res = {"library": _lib.library_path(), "cases": {}}
    for P in (1, 65, 209, 257):
        inp = T._scene(T.SEEDS[P])
        g = T._gaussians(P)
        sets = {"plain": g, "offset17": T._shifted(g, 17)}
        if P >= 192:
            sets["wave1_culled"] = T._cull(g, (torch.arange(P) // 64) == 1)
        for sname, gs in sets.items():
            for vname, use_sh, train in T.VARIANTS:
                res["cases"]["P%d/%s/%s" % (P, sname, vname)] = one_case(gs, inp, use_sh, train)
    inp = T._scene(T.SEEDS[65], width=16, height=16)            # one tile
    g = T._gaussians(65, inp)
    for vname, use_sh, train in T.VARIANTS:
        res["cases"]["P65/one_tile/%s" % vname] = one_case(g, inp, use_sh, train)
    for P in (209, 257):                                       # covariances formed from (scale, rotation)
        inp = T._scene(T.SEEDS[P])
        g = T._gaussians(P)
        for sname, gs in (("plain", g), ("offset17", T._shifted(g, 17)), ("spread", T._spread(g))):
            for train in (True, False):
                res["cases"]["P%d/scale_rot_%s/%s" % (P, sname, "train" if train else "forward_only")] = one_case(gs, inp, True, train, from_sr=True)
    renderer_cases(res)
    inp = scene_inputs("C3")
    inp["scales"], inp["rots"] = inp["means3D"], inp["means3D"]      # (unused: cov6 is given)
    g = {k: inp[k] for k in T.KEYS}
    for vname, use_sh, train in T.VARIANTS:
        res["cases"]["C3/cam0/%s" % vname] = one_case(g, inp, use_sh, train)
    json.dump(res, open(out_path, "w"), indent=1)
    print("%d cases digested with %s" % (len(res["cases"]), res["library"]))


def compare(a_path, b_path):
    a, b = json.load(open(a_path)), json.load(open(b_path))
    print("A: %s\nB: %s" % (a["library"], b["library"]))
    bad = 0
    if sorted(a["cases"]) != sorted(b["cases"]):
        print("DIFFERENT CASE SETS")
        bad += 1
    for name in sorted(a["cases"]):
        ca, cb = a["cases"][name], b["cases"].get(name, {})
        diff = [k for k in ca if ca[k] != cb.get(k)]
        bad += len(diff)
        print("%-36s %s" % (name, "identical (%d outputs)" % len(ca) if not diff else "DIFFERS in " + ", ".join(diff)))
    print("%d cases, %d differing outputs" % (len(a["cases"]), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "digest":
        sys.exit(digest(sys.argv[2]))
    if len(sys.argv) >= 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    sys.exit(__doc__)
