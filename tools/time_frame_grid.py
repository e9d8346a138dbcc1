"""The frame grid (d3ga_amd/frame_grid.py) against the detour it replaces, on the GPU: the six-panel grid of test.py:145-182 and
the three single images of test.py:184-195 at 747 x 1022 and 1080 x 1920.

    python tools/time_frame_grid.py [--iters 100] [--warmup 20] [--out DIR] [--name N] [--kernel-only]   -> DIR/N.json (default profiles/)

The reference side is the reference's lines as they stand MINUS cv2.putText itself (cv2 is not installed here): per panel
`permute -> cpu -> numpy -> ascontiguousarray.astype(float32) -> from_numpy -> permute -> to(device)` (utils/text_helpers.py:
27-50), then th.cat, F.pad and save_image's `mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", uint8)`.  It therefore
UNDERCOUNTS what the reference spends: no glyph is drawn and no PNG is encoded on either side.

Figures, the two sides alternating call by call in one process, median / p10 / p90:
  device_us    device events around the enqueue of our one launch (compose_grid / to_uint8 with out=)
  to_host_ms   wall clock until the uint8 image is on the host: ours = the launch + GridWriter.submit + handle.numpy();
               reference = the lines above (they end on the host by themselves)
  in_graph_us  the kernel alone: a replayed graph of at least 20 calls that ROTATE over `in_graph_sets` independent copies of the
               inputs and the output, 768 MB per lap, so that the 256 MB Infinity Cache holds nothing a launch reads; per call.
               `share_of_8TBps` is the time its algorithmic bytes (4 C h w per panel read + the output written) need at 8 TB/s
               over that figure.  `in_graph_us_same_buffers`: 20 identical launches over ONE set, which may be served from the
               cache -- recorded to show the difference, not used for the share.
device_us is taken for our side only (the reference synchronises inside its own lines, so events around it measure nothing
else than its wall clock); the two sides alternate in the wall-clock figure.  `--kernel-only --name NAME` with D3GA_LIB_PATH set
records the in-graph figures of an A/B build (the workgroup shapes of DESIGN 4.4o).  No threshold is set on any of these
numbers: they are recorded, not asserted."""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from time_calib import alternate, graph_time, stats  # noqa: E402  (tools/ is the script's directory)

SIZES = [(747, 1022), (1080, 1920)]
PEAK_BYTES_PER_S = 8.0e12
ROTATE_BYTES = 3 * 256 * 2 ** 20          # what one lap of the in-graph measurement touches: three Infinity Caches
NAMES = [["Prediction", "Input upper", "Input lower"], ["3D Means", "Deformed upper", "Deformed lower"]]


def wall_alternate(fns, iters, warmup):
    """name -> ms per call (array), wall clock with a synchronisation in front of every call"""
    out = {n: [] for n in fns}
    for i in range(warmup + iters):
        for n, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            if i >= warmup:
                out[n].append((time.perf_counter() - t0) * 1e3)
    return {n: np.array(v) for n, v in out.items()}


def ms_stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "p10_ms": round(float(np.percentile(ms, 10)), 3),
            "p90_ms": round(float(np.percentile(ms, 90)), 3)}


def reference_write_text(img):
    """utils/text_helpers.py:27-50 around the cv2.putText call"""
    device = img.device
    host = img.permute(1, 2, 0).cpu().numpy()
    host = np.ascontiguousarray(host).astype(np.float32)
    return torch.from_numpy(host).permute(2, 0, 1).to(device)


def reference_save(image):
    """torchvision.utils.save_image up to the array it hands to PIL"""
    return image.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).numpy()


def algorithmic_bytes(panels, out):
    return sum(4 * p.C * p.h * p.w for p in panels) + out.numel() * out.element_size()


def fresh(rows):
    """the same rows over NEW device memory: every panel's image cloned (the sources are contiguous, strides stay)"""
    out = []
    for row in rows:
        out.append([])
        for p in row:
            q = copy.copy(p)
            q.img = p.img.clone()
            out[-1].append(q)
    return out


def rotating(rows, out, kw, nbytes):
    """-> (fn, calls): fn composes set i, i + 1, ... of enough independent copies of (inputs, output) that one lap touches
    ROTATE_BYTES -- three times the 256 MB Infinity Cache -- so no launch finds its data cached by the launch before it"""
    from d3ga_amd.frame_grid import compose_grid
    sets = int(min(96, max(2, -(-ROTATE_BYTES // nbytes))))
    pool = [(rows, out)] + [(fresh(rows), torch.empty_like(out)) for _ in range(sets - 1)]
    turn = [0]

    def fn():
        r, o = pool[turn[0] % sets]
        turn[0] += 1
        compose_grid(r, out=o, **kw)
    return fn, sets * max(1, -(-20 // sets)), sets


def measure(name, rows, kw, reference, writer, iters, warmup, kernel_only):
    """one written image: compose_grid(rows, **kw); `reference` returns the host array"""
    from d3ga_amd.frame_grid import compose_grid
    out, path = compose_grid(rows, return_path=True, **kw)
    ours = lambda: compose_grid(rows, out=out, **kw)
    panels = [p for row in rows for p in row]
    rec = {"path": path, "out_shape": list(out.shape), "bytes": algorithmic_bytes(panels, out)}
    if not kernel_only:
        def to_host():
            ours()
            return writer.submit(out).numpy()
        got, want = to_host(), reference()
        rec["max_abs_difference_outside_text"] = int(np.abs(got[-8:].astype(np.int32) - want[-8:].astype(np.int32)).max())
        rec["device_us"] = stats(alternate({"hip": ours}, iters, warmup)["hip"])          # our side only: the reference synchronises
        ms = wall_alternate({"hip": to_host, "reference": reference}, iters, warmup)
        rec["to_host_ms"] = {k: ms_stats(v) for k, v in ms.items()}
    fn, calls, sets = rotating(rows, out, kw, rec["bytes"])
    us = graph_time(fn, calls=calls)
    rec["in_graph_us"] = round(us, 2)
    rec["in_graph_sets"] = sets
    rec["share_of_8TBps"] = round(rec["bytes"] / PEAK_BYTES_PER_S / (us * 1e-6), 4)
    rec["in_graph_us_same_buffers"] = round(graph_time(ours), 2)
    if path == "vector":                                     # the same launches on the one-pixel-per-thread kernel
        fn, calls, _ = rotating(rows, out, dict(kw, force_scalar=True), rec["bytes"])
        rec["in_graph_us_scalar_path"] = round(graph_time(fn, calls=calls), 2)
    print(name, rec)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--name", default="frame_grid_timing", help="file name of the record, without .json")
    ap.add_argument("--kernel-only", action="store_true", help="the in-graph figures alone (A/B builds selected by D3GA_LIB_PATH)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    from d3ga_amd import library_path
    from d3ga_amd.frame_grid import GridWriter, Panel
    os.makedirs(a.out, exist_ok=True)
    rec = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "peak_bytes_per_s": PEAK_BYTES_PER_S,
           "library": os.path.basename(library_path()), "rotate_bytes": ROTATE_BYTES,
           "reference_side": "the reference's lines minus cv2.putText and the PNG encoder: it undercounts"}
    writer = GridWriter(depth=2)
    for h, w in SIZES:
        g = torch.Generator().manual_seed(h)
        imgs = [[torch.rand(3, h, w, generator=g).cuda() for _ in range(3)] for _ in range(2)]
        rgba, heat = torch.rand(4, h, w, generator=g).cuda(), torch.rand(3, h, w, generator=g).cuda()
        cell = torch.tensor([31.0625], device="cuda")
        size = {}

        rows = [[Panel(imgs[r][k], NAMES[r][k]) for k in range(3)] for r in range(2)]

        def reference_grid():
            image = torch.cat([torch.cat([reference_write_text(t) for t in row], dim=2) for row in imgs], dim=1)
            _, hh, ww = image.shape
            image = torch.nn.functional.pad(image, (0, ww % 2, 0, hh % 2), "constant", 1)
            return reference_save(image)
        size["grid"] = measure(f"{h}x{w} grid", rows, {}, reference_grid, writer, a.iters, a.warmup, a.kernel_only)

        singles = {"prediction": (Panel(imgs[0][0]), 3, lambda: reference_save(imgs[0][0])),
                   "ground_truth_rgba": (Panel(rgba), 4, lambda: reference_save(rgba)),
                   "heatmap": (Panel(heat, "{:.3f} (dB)", color=(1, 1, 1), value=cell), 3, lambda: reference_save(reference_write_text(heat)))}
        for name, (panel, channels, ref) in singles.items():
            size[name] = measure(f"{h}x{w} {name}", [[panel]], dict(channels=channels, pad_even=False), ref, writer, a.iters, a.warmup,
                                 a.kernel_only)
        rec[f"{h}x{w}"] = size
    json.dump(rec, open(os.path.join(a.out, a.name + ".json"), "w"), indent=1)


if __name__ == "__main__":
    main()
