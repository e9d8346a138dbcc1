"""Sample preparation (d3ga_amd/sample_prep.py) on the GPU, beside the bytes it has to move and beside the host lines it replaces.

    python tools/time_sample_prep.py [--iters 100] [--warmup 20] [--host-iters 5] [--out DIR] [--name N]
        -> DIR/N.json (default profiles/sample_prep_timing.json)

ActorsHQ mode at 747 x 1022 and 1920 x 1080 (W x H), B = 1 and 4, uint8 and float32 image; Goliath mode from 1494 x 2044 to the
747 x 1022 frame, B = 1.  Figures per case:
  eager_us        device events around prepare_*(..., out=slots): one launch, median / p10 / p90
  in_graph_us     a replayed graph of at least 20 calls that ROTATE over `in_graph_sets` independent sets of inputs and outputs,
                  768 MB per lap, so that the 256 MB Infinity Cache holds nothing a launch reads or writes; per call
  in_graph_us_same_buffers   the same with one set: what a captured step sees when its slots stay cache-resident
  algorithmic_bytes, hbm_floor_us, roofline_share   7 bytes read per pixel (image 3, part image 3, matte 1) plus 15 (uint8 image:
                  3 + 4 + 4 + 4) or 24 (float32: 12 + 12) written, over 8 TB/s, against in_graph_us.  Goliath: 4 bytes read per
                  input pixel, 24 written per output pixel
  upload_bytes    per frame over the bus: the three decoded arrays (7 bytes per pixel; 9 when the matte travels as the (H,W,3) array
                  imread returns) against the loader's float32 image, int32 labels and two bool planes (18)
  host_numpy_ms   the numpy lines of the loader that the launch replaces, restated here operation for operation (flip, cast and
                  transpose twice; threshold; boundary; the float64 label arithmetic; four masked fills; the int32 cast), WITHOUT
                  the two cv2 morphology calls (cv2 is absent), one thread, on this box's CPU, median of --host-iters
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
SIZES = [(747, 1022), (1920, 1080)]                          # (W, H)
GOLIATH_IN = (1494, 2044)                                    # (W, H): halves to the 747 x 1022 frame


def synthetic_sample(B, H, W, seed):
    """A person-sized matte with a soft rim, a part image in the four part colours, an image of noise: uint8, on the host"""
    g = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
    d = (xx / 0.45) ** 2 + (yy / 0.85) ** 2
    matte = np.clip((1.05 - d) * 900, 0, 255).astype(np.uint8)
    palette = np.array([[0, 0, 255], [0, 255, 0], [255, 0, 0], [127, 127, 127]], np.uint8)      # BGR
    seg = palette[np.clip(((yy + 1) * 2).astype(np.int64), 0, 3)] * (d < 1.0)[..., None].astype(np.uint8)
    image = g.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    return image, np.broadcast_to(seg, (B, H, W, 3)).copy(), np.broadcast_to(matte, (B, H, W)).copy()


def numpy_lines(image_bgr, seg_bgr, matte):
    """One frame through the loader's numpy operations (no morphology): what a worker thread spends per sample"""
    image = np.transpose(image_bgr[..., ::-1].astype(np.float32), axes=(2, 0, 1))
    _, H, W = image.shape
    seg = np.transpose(seg_bgr[..., ::-1].astype(np.float32), axes=(2, 0, 1))[:, :H, :W]
    kept = matte.copy()
    m = matte.copy()
    m[m < 128] = 0
    m[m > 128] = 1
    er, di = m.copy(), m.copy()                              # stand-ins for the two cv2 calls: their cost is not counted
    boundary = np.logical_or((di - er) == 1, np.logical_and(kept > 5, kept < 250))
    fg = (m == 1)[None]
    on = fg > 0
    parts = seg * on
    has = (parts.sum(axis=0) > 0)[None]
    parts = parts + (on * 127) * (1 - has) * on
    picks = [parts[0] == 255, parts[1] == 255, parts[2] == 255, parts[0] == 127]
    label = np.zeros([1, H, W])
    for value, pick in enumerate(picks, start=1):
        label[pick[None]] = value
    return image, label.astype(np.int32), fg, boundary[None]


def rotating(make_call, per_set_bytes):
    sets = int(min(96, max(2, -(-ROTATE_BYTES // per_set_bytes))))
    calls = [make_call() for _ in range(sets)]
    turn = [0]

    def rotate():
        calls[turn[0] % sets]()
        turn[0] += 1
    return rotate, sets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=5)
    ap.add_argument("--name", default="sample_prep_timing", help="file name of the record, without .json")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    from d3ga_amd import library_path
    from d3ga_amd.sample_prep import prepare_actorshq, prepare_goliath
    os.makedirs(a.out, exist_ok=True)
    rec = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "library": os.path.basename(library_path()),
           "rotate_bytes": ROTATE_BYTES, "hbm_bytes_per_s": HBM_BYTES_PER_S, "cpus_allowed": len(os.sched_getaffinity(0)), "actorshq": {}}
    for W, H in SIZES:
        host_image, host_seg, host_matte = synthetic_sample(1, H, W, W)
        ms = []
        for _ in range(a.host_iters + 1):
            t0 = time.perf_counter()
            numpy_lines(host_image[0], host_seg[0], host_matte[0])
            ms.append((time.perf_counter() - t0) * 1e3)
        host_ms = round(float(np.median(ms[1:])), 2)
        for B in (1, 4):
            image, seg, matte = (torch.from_numpy(np.ascontiguousarray(np.broadcast_to(x, (B,) + x.shape[1:]))).cuda()
                                 for x in (host_image, host_seg, host_matte))
            for dtype, written in ((torch.uint8, 15), (torch.float32, 24)):
                def make_call(src=None):
                    i, s, m = src or (image.clone(), seg.clone(), matte.clone())
                    out = {"image": torch.empty(B, 3, H, W, dtype=dtype, device="cuda"), "seg_part": torch.empty(B, 1, H, W, dtype=torch.int32, device="cuda"),
                           "seg_fg": torch.empty(B, 1, H, W, device="cuda"), "boundary_fg": torch.empty(B, 1, H, W, device="cuda")}
                    return lambda: prepare_actorshq(i, s, m, out=out)
                ours = make_call((image, seg, matte))
                nbytes = (7 + written) * B * H * W
                r = {"size": [W, H], "B": B, "image_dtype": str(dtype).replace("torch.", ""), "path": "vector" if W % 4 == 0 else "scalar",
                     "eager_us": stats(alternate({"hip": ours}, a.iters, a.warmup)["hip"])}
                rotate, sets = rotating(make_call, nbytes)
                r["in_graph_us"] = round(graph_time(rotate, calls=sets * max(1, -(-20 // sets))), 2)
                r["in_graph_sets"] = sets
                r["in_graph_us_same_buffers"] = round(graph_time(ours), 2)
                floor = nbytes / HBM_BYTES_PER_S * 1e6
                r.update({"algorithmic_bytes": nbytes, "hbm_floor_us": round(floor, 2), "roofline_share": round(floor / r["in_graph_us"], 3),
                          "achieved_TBps": round(nbytes / r["in_graph_us"] * 1e-6, 3),
                          "upload_bytes": {"decoded_uint8": 7 * B * H * W, "decoded_uint8_matte_bgr": 9 * B * H * W, "loader_tensors": 18 * B * H * W},
                          "host_numpy_ms_per_frame": host_ms, "host_numpy_ms": round(host_ms * B, 2)})
                rec["actorshq"][f"{W}x{H}_B{B}_{r['image_dtype']}"] = r
                print(json.dumps(r))
                del rotate
                torch.cuda.empty_cache()
    W, H = GOLIATH_IN
    g = torch.Generator().manual_seed(3)
    image = torch.randint(0, 256, (1, 3, H, W), generator=g, dtype=torch.uint8)
    parts = (torch.randint(0, 30, (1, 1, H, W), generator=g, dtype=torch.uint8) * (torch.rand(1, 1, H, W, generator=g) < 0.5)).to(torch.uint8)
    ms = []
    for _ in range(a.host_iters + 1):
        t0 = time.perf_counter()
        for x in (image[0].float(), parts[0].float(), (parts[0] != 0.0).to(torch.float32)):
            torch.nn.functional.interpolate(x[None], scale_factor=0.5, mode="bilinear")
        ms.append((time.perf_counter() - t0) * 1e3)
    image, parts = image.cuda(), parts.cuda()

    def make_goliath(src=None):
        i, p = src or (image.clone(), parts.clone())
        out = {n: torch.empty(1, c, H // 2, W // 2, device="cuda") for n, c in (("image", 3), ("seg_part", 1), ("seg_fg", 1), ("boundary_fg", 1))}
        return lambda: prepare_goliath(i, p, out=out)
    ours = make_goliath((image, parts))
    nbytes = 4 * H * W + 24 * (H // 2) * (W // 2)
    r = {"size_in": [W, H], "size_out": [W // 2, H // 2], "B": 1, "path": "vector" if (W // 2) % 4 == 0 else "scalar",
         "eager_us": stats(alternate({"hip": ours}, a.iters, a.warmup)["hip"])}
    rotate, sets = rotating(make_goliath, nbytes)
    r["in_graph_us"] = round(graph_time(rotate, calls=sets * max(1, -(-20 // sets))), 2)
    r["in_graph_sets"] = sets
    r["in_graph_us_same_buffers"] = round(graph_time(ours), 2)
    floor = nbytes / HBM_BYTES_PER_S * 1e6
    r.update({"algorithmic_bytes": nbytes, "hbm_floor_us": round(floor, 2), "roofline_share": round(floor / r["in_graph_us"], 3),
              "achieved_TBps": round(nbytes / r["in_graph_us"] * 1e-6, 3),
              "upload_bytes": {"decoded_uint8": 4 * H * W, "loader_tensors": 24 * (H // 2) * (W // 2)},
              "host_torch_interpolate_ms": round(float(np.median(ms[1:])), 2), "host_threads": torch.get_num_threads()})
    rec["goliath"] = r
    print(json.dumps(r))
    json.dump(rec, open(os.path.join(a.out, a.name + ".json"), "w"), indent=1)


if __name__ == "__main__":
    main()
