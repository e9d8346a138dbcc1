"""The PNG encoder (d3ga_amd/png.py) against the path it replaces, on the GPU: the uint8 image copied to the host and encoded
there by a CPU thread, as torchvision.utils.save_image (test.py:182-195) and cv2.imwrite (train.py:371) do.

    python tools/time_png.py [--iters 50] [--warmup 10] [--out DIR] [--name N]   -> DIR/N.json (default profiles/png_timing.json)

Shapes: 1080 x 1920 RGB, the 747 x 1022 Goliath frame in RGB and RGBA, and the three-panel grid of test.py (748 x 3066 RGB).  The
picture is a white background with a textured body, seeded.

Figures per shape:
  eager_us       device events around encode_png(img, out=buf): two launches, median / p10 / p90
  in_graph_us    a replayed graph of at least 20 calls that ROTATE over `in_graph_sets` independent (image, PngBuffer) pairs, 768 MB
                 per lap, so that the 256 MB Infinity Cache holds nothing a launch reads; per call
  to_host_ms     wall clock until the file's bytes are on the host: encode_png + GridWriter.submit_png + handle.tobytes()
  file_bytes     ours; `host_file_bytes` the host encoder's
  host_*         the parent's path for the same image: GridWriter.submit + handle.numpy() + PIL.Image.save at its default level
                 (zlib level 6), or -- where PIL is absent -- zlib.compress(filtered bytes, 6), which is its core, the filtered
                 bytes being those of our own file.  `host_one_thread_ms`: one thread, median; `host_pool10_ms_per_image`: wall
                 clock of 20 images through a pool of ten threads, per image (the machines allow a command 16 CPUs).
  size_vs_zlib_rle  (recorded once, on the CPU side of the run) is in DESIGN.md 4.4p; this tool measures time.
No threshold is set on any of these numbers: they are recorded, not asserted."""
import argparse
import io
import json
import os
import struct
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from time_calib import alternate, graph_time, stats  # noqa: E402  (tools/ is the script's directory)

ROTATE_BYTES = 3 * 256 * 2 ** 20
SHAPES = {"1080x1920_rgb": (1080, 1920, 3, 1), "747x1022_rgb": (747, 1022, 3, 1), "747x1022_rgba": (747, 1022, 4, 1),
          "test_grid_748x3066_rgb": (748, 1022, 3, 3)}


def body_on_white(H, W, C, seed, device):
    """uint8 (H, W, C): a white background with a textured body; alpha (C = 4) is the body's mask"""
    g = torch.Generator().manual_seed(seed)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    body = ((x - W / 2) / (0.28 * W)) ** 2 + ((y - H / 2) / (0.42 * H)) ** 2 < 1
    tex = 128 + 60 * (torch.sin(x / 7.0) * torch.cos(y / 5.0))[..., None] + 12 * torch.randn(H, W, 3, generator=g)
    img = torch.where(body[..., None], tex.clamp(0, 255), torch.full_like(tex, 255.0)).to(torch.uint8)
    if C == 4:
        img = torch.cat([img, (body[..., None] * 255).to(torch.uint8)], dim=2)
    return img.contiguous().to(device)


def filtered_bytes(png):
    """the filtered bytes inside a PNG file: its IDAT chunks inflated"""
    at, data = 8, []
    while at < len(png):
        n, = struct.unpack(">I", png[at:at + 4])
        if png[at + 4:at + 8] == b"IDAT":
            data.append(png[at + 8:at + 8 + n])
        at += 12 + n
    return zlib.decompress(b"".join(data))


def host_encoder(png):
    """(name, fn(array) -> bytes): PIL at its default level, or zlib level 6 over our file's filtered bytes"""
    try:
        from PIL import Image

        def pil(arr):
            b = io.BytesIO()
            Image.fromarray(arr if arr.shape[2] > 1 else arr[:, :, 0]).save(b, format="PNG")
            return b.getvalue()
        return "PIL.Image.save, default level", pil
    except ImportError:
        filt = filtered_bytes(png)
        return "zlib.compress(filtered, 6)", lambda arr: zlib.compress(filt, 6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-iters", type=int, default=5)
    ap.add_argument("--name", default="png_timing", help="file name of the record, without .json")
    ap.add_argument("--rows", type=int, default=0, help="rows_per_strip (0: the default)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    from d3ga_amd import GridWriter, PngBuffer, encode_png, library_path, png_bytes
    os.makedirs(a.out, exist_ok=True)
    rec = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "library": os.path.basename(library_path()),
           "rotate_bytes": ROTATE_BYTES, "rows_per_strip": a.rows, "cpus_allowed": len(os.sched_getaffinity(0))}
    writer = GridWriter(depth=2)
    for name, (H, W, C, across) in SHAPES.items():
        img = torch.cat([body_on_white(H, W, C, 7 + k, "cuda") for k in range(across)], dim=1).contiguous()
        H, W, C = img.shape
        buf = PngBuffer(H, W, C, a.rows)
        ours = lambda: encode_png(img, out=buf)
        ours()
        data = png_bytes(buf)
        r = {"shape": [H, W, C], "file_bytes": len(data), "raw_bytes": img.numel(), "capacity": buf.capacity, "scratch_bytes": buf.scratch_bytes}
        r["eager_us"] = stats(alternate({"hip": ours}, a.iters, a.warmup)["hip"])
        per_set = img.numel() + buf.storage.numel()
        sets = int(min(96, max(2, -(-ROTATE_BYTES // per_set))))
        pool = [(img, buf)] + [(img.clone(), PngBuffer(H, W, C, a.rows)) for _ in range(sets - 1)]
        turn = [0]

        def rotate():
            i, b = pool[turn[0] % sets]
            turn[0] += 1
            encode_png(i, out=b)
        r["in_graph_us"] = round(graph_time(rotate, calls=sets * max(1, -(-20 // sets))), 2)
        r["in_graph_sets"] = sets
        r["in_graph_us_same_buffers"] = round(graph_time(ours), 2)
        del pool

        def to_host():
            ours()
            return writer.submit_png(buf).tobytes()
        assert to_host() == data
        ms = []
        for i in range(a.warmup + a.iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            to_host()
            if i >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        r["to_host_ms"] = {"median_ms": round(float(np.median(ms)), 3), "p10_ms": round(float(np.percentile(ms, 10)), 3),
                           "p90_ms": round(float(np.percentile(ms, 90)), 3)}
        # the parent's path: the image over the bus, a CPU thread encodes
        r["host_encoder"], encode = host_encoder(data)

        def parent():
            return encode(writer.submit(img).numpy())
        r["host_file_bytes"] = len(parent())
        ms = []
        for _ in range(a.host_iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            parent()
            ms.append((time.perf_counter() - t0) * 1e3)
        r["host_one_thread_ms"] = round(float(np.median(ms)), 2)
        arr = writer.submit(img).numpy()
        with ThreadPoolExecutor(10) as ex:
            t0 = time.perf_counter()
            list(ex.map(encode, [arr] * 20))
            r["host_pool10_ms_per_image"] = round((time.perf_counter() - t0) * 1e3 / 20, 2)
        print(name, r, flush=True)
        rec[name] = r
    json.dump(rec, open(os.path.join(a.out, a.name + ".json"), "w"), indent=1)


if __name__ == "__main__":
    main()
