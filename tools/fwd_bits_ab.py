#!/usr/bin/env python3
"""Bit-for-bit comparison of the compositing forward's outputs between two builds of the library.

One process loads ONE library (D3GA_LIB_PATH, or the shipped one), so the comparison is two runs and a compare:

    D3GA_LIB_PATH=tools/_build/libd3ga_hip_parent.so python tools/fwd_bits_ab.py digest bits_parent.json
    python tools/fwd_bits_ab.py digest bits_new.json
    python tools/fwd_bits_ab.py compare bits_parent.json bits_new.json      # exit 1 on any differing digest

`digest` renders, with grad enabled (so that the forward writes the per-block lists), the bench's eight C3 cameras and camera 0 of
T1, C1 and C5 (the whole 4K frame) through the entry points below and stores a SHA-256 of every output's bytes:
  plain (render), l1 (render_l1: the headline's kernel, + the loss value), depth (the rasterizer with its inverse-depth image),
  pair (render_pair: DUAL), pair_depth (DUAL + DEPTH): colour image(s), inverse depth, final_T, n_contrib, blk_count and the USED
  prefix of every block's list (rows 16 begin + b (end - begin) + [0, blk_count[t, b]) of blk_list; the rest is uninitialised);
  views4 / views4_bg (render_views, k = 4 cameras, shared / per-view background, with targets): the colour images and the loss
  (the view-batched image scratch is not reachable from Python).
"""
import hashlib
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def scratch_digests():
    import torch
    from d3ga_amd import rasterizer as R
    W, H = R._last_img[torch.cuda.current_device()][1:3]                     # the raster of the most recent forward
    T, n = R.last_termination()
    cnt, lst = R.last_block_lists()
    tile_start = R.last_tile_lists(W, H)[0]
    gx, gy = (W + 15) // 16, (H + 15) // 16
    begin, length = tile_start[:-1], tile_start[1:] - tile_start[:-1]
    dev = cnt.device
    # the forward writes the counts of quadrants that start inside the image; the others are uninitialised: count them as 0
    t = torch.arange(gx * gy, device=dev).view(-1, 1)
    q = (torch.arange(16, device=dev) >> 2).view(1, 16)
    written = ((t % gx) * 16 + 8 * (q & 1) < W) & ((t // gx) * 16 + 8 * (q >> 1) < H)
    cnt = torch.where(written, cnt, torch.zeros_like(cnt))
    if bool(((cnt < 0) | (cnt > length.view(-1, 1))).any()):
        raise RuntimeError("blk_count outside [0, list length]")
    b = torch.arange(16, device=dev).view(1, 16)
    first = 16 * begin.view(-1, 1) + b * length.view(-1, 1)                  # first row of block b of tile t
    total = int(cnt.sum())
    # row index of every used entry: first[t, b] + (0 .. cnt[t, b] - 1), tiles and blocks in order
    flat_first, flat_cnt = first.reshape(-1), cnt.reshape(-1)
    owner = torch.repeat_interleave(torch.arange(flat_cnt.numel(), device=dev), flat_cnt)
    starts = torch.cumsum(flat_cnt, 0) - flat_cnt
    rows = flat_first[owner] + (torch.arange(total, device=dev) - starts[owner])
    return {"final_T": sha(T), "n_contrib": sha(n), "blk_count": sha(cnt), "blk_list_used": sha(lst[rows]), "blk_used_entries": total}


def digest(out_path):
    import torch
    import d3ga_amd.renderer as RD
    from d3ga_amd import _lib, synthetic as syn
    from d3ga_amd.cage_deform import canonical_gradient, lbs_cage_deform
    from d3ga_amd.raster_views import CameraBatch
    dev = torch.device("cuda")
    res = {"library": _lib.library_path(), "cases": {}}
    captured = {}

    def depth_on(fn):
        def wrapped(*a, **k):
            k["want_invdepth"] = True
            out = fn(*a, **k)
            captured["invdepth"] = out[2]
            return out
        return wrapped
    plain_op, pair_op = RD.rasterize_gaussians, RD.rasterize_gaussians_pair
    for wl_name, cams in (("T1", [0]), ("C1", [0]), ("C3", list(range(8))), ("C5", [0])):
        sc = syn.make_scene(wl_name)
        wl = sc["workload"]
        d = lambda t: t.to(dev)
        canon, tetras, tetra_id = d(sc["canon_points"]), d(sc["tetras"]), d(sc["tetra_id"])
        P = sc["barys"].shape[0]
        with torch.no_grad():
            means, cov6, _ = lbs_cage_deform(canon, d(sc["delta_node"]), d(sc["joint_mats"]), d(sc["skin_idx"]), d(sc["skin_w"]), tetras, tetra_id,
                                             d(sc["barys"]), canonical_gradient(canon, tetras, tetra_id).contiguous(), d(sc["scaling"]),
                                             d(sc["rotation"]), delta_barys=torch.zeros(P, 4, device=dev), scale_activation="exp")
        pkg = {"means3D": means.detach().requires_grad_(True), "cov3D_precomp": cov6.detach().requires_grad_(True),
               "opacity_logits": d(sc["opacity_logit"]).requires_grad_(True),
               "shs": d(torch.cat([sc["features_dc"], sc["features_rest"]], 1)).requires_grad_(True), "rgb": None, "sh_degree": wl.sh_degree}
        g = torch.Generator().manual_seed(7)
        colors2 = torch.rand(P, 3, generator=g).to(dev)
        bg, bg2 = torch.ones(3, device=dev), torch.zeros(3, device=dev)
        W, H = wl.width, wl.height
        batches, targets = [], []
        for v in cams:
            batches.append(syn.make_batch(W, H, azimuth=2 * math.pi * v / 8, camera_id=v, fill=0.85))
            targets.append(torch.rand(3, H, W, generator=torch.Generator().manual_seed(100 + v)).to(dev))
        for v, batch, target in zip(cams, batches, targets):
            def put(kind, extra):
                torch.cuda.synchronize()
                extra.update(scratch_digests())
                res["cases"]["%s/cam%d/%s" % (wl_name, v, kind)] = extra
            o = RD.render(batch, pkg, bg)
            put("plain", {"render": sha(o["render"])})
            o = RD.render_l1(batch, pkg, bg, target)
            put("l1", {"render": sha(o["render"]), "l1": sha(o["l1"])})
            o = RD.render_pair(batch, pkg, bg, colors2, bg2)
            put("pair", {"render": sha(o["render"]), "render2": sha(o["render2"])})
            RD.rasterize_gaussians, RD.rasterize_gaussians_pair = depth_on(plain_op), depth_on(pair_op)
            try:
                o = RD.render(batch, pkg, bg)
                put("depth", {"render": sha(o["render"]), "invdepth": sha(captured["invdepth"])})
                o = RD.render_pair(batch, pkg, bg, colors2, bg2)
                put("pair_depth", {"render": sha(o["render"]), "render2": sha(o["render2"]), "invdepth": sha(captured["invdepth"])})
            finally:
                RD.rasterize_gaussians, RD.rasterize_gaussians_pair = plain_op, pair_op
        if len(cams) >= 4:
            for first in range(0, len(cams), 4):
                cb = CameraBatch(4, W, H, device=dev).set(batches[first:first + 4])
                tg = torch.stack(targets[first:first + 4]).contiguous()
                bgk = torch.rand(4, 3, generator=torch.Generator().manual_seed(3)).to(dev)
                for kind, b in (("views4", bg), ("views4_bg", bgk)):
                    o = RD.render_views(None, pkg, b, targets=tg, cameras=cb)
                    torch.cuda.synchronize()
                    res["cases"]["%s/cam%d-%d/%s" % (wl_name, first, first + 3, kind)] = {"render": sha(o["render"]), "l1": sha(o["l1"])}
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
        print("%-28s %s" % (name, "identical (%s)" % ", ".join(sorted(ca)) if not diff else "DIFFERS in " + ", ".join(diff)))
    print("%d cases, %d differing outputs" % (len(a["cases"]), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "digest":
        sys.exit(digest(sys.argv[2]))
    if len(sys.argv) >= 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    sys.exit(__doc__)
