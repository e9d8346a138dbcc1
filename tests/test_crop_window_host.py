"""Host side of crop-window rasterization (include/d3ga.h: D3GA_CAMERA_SLOT_WINDOWED): the crop -> (w, h, ox, oy) mapping against
renderer.paste, the windowed camera-row layout, the new size queries, and the refusals.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _batch(W, H, cx, cy):
    from d3ga_amd import synthetic as syn
    return syn.make_batch(W, H, cx=cx, cy=cy)


def test_crop_window_matches_paste_on_random_crops():
    from d3ga_amd.cameras import crop_window
    from d3ga_amd.renderer import paste
    rng = np.random.default_rng(0)
    for _ in range(300):
        W, H = int(rng.integers(8, 300)), int(rng.integers(8, 300))
        b = _batch(W, H, int(rng.integers(0, W + 1)), int(rng.integers(0, H + 1)))
        w, h, ox, oy, W2, H2 = crop_window(b)
        assert (w, h) == (b["width"], b["height"]) and (W2, H2) == (W, H)
        img = torch.arange(3 * h * w, dtype=torch.float32).view(3, h, w)
        assert torch.equal(paste(img, b["crop"]), img[:, oy:oy + H, ox:ox + W])


def test_crop_window_on_the_golden_boundary_cases():
    from d3ga_amd.cameras import crop_window
    from d3ga_amd.renderer import paste
    z = np.load(os.path.join(ROOT, "tests", "golden", "boundary_cases.npz"), allow_pickle=True)
    n = 0
    for key in (k for k in z.files if k.endswith("_crop")):
        row = np.asarray(z[key], dtype=np.float64).reshape(6)
        w, h = (int(x) for x in np.asarray(z[key[:-len("crop")] + "batch_wh"]).reshape(2))
        W, H = int(row[4]), int(row[5])
        if not (0 < W <= w and 0 < H <= h):
            continue
        b = {"width": w, "height": h, "crop": row}
        _, _, ox, oy, _, _ = crop_window(b)
        img = torch.arange(h * w, dtype=torch.float32).view(1, h, w)
        assert torch.equal(paste(img, b["crop"]), img[:, oy:oy + H, ox:ox + W])
        n += 1
    # the golden file's crops (if any) and, always, the four paste branches at the edges of the padding
    for W, H, cx, cy in [(100, 80, 0, 0), (100, 80, 100, 80), (100, 80, 50, 40), (101, 79, 51, 39), (101, 79, 50, 40)]:
        b = _batch(W, H, cx, cy)
        w, h, ox, oy, _, _ = crop_window(b)
        img = torch.arange(h * w, dtype=torch.float32).view(1, h, w)
        assert torch.equal(paste(img, b["crop"]), img[:, oy:oy + H, ox:ox + W])
        n += 1
    assert n >= 5


def test_header_declares_the_windowed_slot_and_the_new_queries():
    src = open(os.path.join(ROOT, "include", "d3ga.h")).read()
    assert re.search(r"#define\s+D3GA_CAMERA_SLOT_WINDOWED\s+\(-1\.0f\)", src)
    assert re.search(r"#define\s+D3GA_CAMERA_SLOT_WINDOWED_FLOATS\s+9\b", src)
    for name in ("d3ga_raster_scratch_bytes_window", "d3ga_raster_binning_layout_window"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
    from d3ga_amd import _lib
    from d3ga_amd.cameras import CAMERA_SLOT_WINDOWED
    assert _lib.CAMERA_SLOT_WINDOWED == CAMERA_SLOT_WINDOWED == -1.0
    assert "d3ga_raster_scratch_bytes_window" in _lib.EXPORTS and "d3ga_raster_binning_layout_window" in _lib.EXPORTS


def test_window_size_queries():
    from d3ga_amd import _lib
    L = _lib.lib()
    W, H, k, cap, P = 197, 150, 3, 5000, 1000
    sw, sv = (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 3)()
    assert L.d3ga_raster_scratch_bytes_window(P, W, H, k, cap, 0, sw) == 0
    assert L.d3ga_raster_scratch_bytes_views(P, W, H, k, cap, 0, sv) == 0
    assert sw[0] == sv[0]                                            # the per-Gaussian records do not depend on the grid
    assert sw[1] > sv[1] and sw[2] > sv[2]                           # one spare tile column and row per view + the window table
    off = (ctypes.c_int64 * 7)()
    assert L.d3ga_raster_binning_layout_window(W, H, k, cap, off) == 0
    assert list(off[:6]) == sorted(off[:6]) and off[6] % 256 == 0 and off[6] + 16 * k <= sw[1]
    tiles = (((W + 15) // 16) + 1) * (((H + 15) // 16) + 1) * k
    assert off[2] - off[1] >= 4 * tiles
    assert L.d3ga_raster_scratch_bytes_window(P, 0, H, k, cap, 0, sw) < 0
    assert L.d3ga_raster_binning_layout_window(W, H, k, cap, None) < 0


def test_windowed_camera_rows_and_slot_layout():
    from d3ga_amd.cameras import Camera, CameraSlot, crop_window, window_row_host
    from d3ga_amd.raster_views import CameraBatch
    b = _batch(200, 152, 131, 99)
    w, h, ox, oy, W, H = crop_window(b)
    row = window_row_host(b)
    m = Camera.pack_host_cached(b)
    assert np.array_equal(row[:53], m) and tuple(row[53:57]) == (w, h, ox, oy)
    slot = CameraSlot.windowed(W, H, device="cpu")
    assert slot.windowed and slot.tanfovx == slot.tanfovy == -1.0
    slot.set(b)
    assert slot.camera_center.numel() == 9
    assert np.array_equal(slot.camera_center.numpy(), row[48:57])
    assert np.array_equal(slot.full_proj_transform.reshape(-1).numpy(), m[32:48])
    cams = CameraBatch(2, W, H, device="cpu", windowed=True).set([b, _batch(200, 152, 70, 60)])
    assert tuple(cams.campos.shape) == (2, 9)
    assert np.array_equal(cams.campos[0].numpy(), row[48:57])
    assert tuple(cams.campos[1, 5:].tolist()) == crop_window(_batch(200, 152, 70, 60))[:4]


def test_refusals():
    from d3ga_amd.cameras import CameraSlot, crop_window
    from d3ga_amd.raster_views import CameraBatch
    from d3ga_amd.renderer import render
    a, other = _batch(200, 152, 131, 99), _batch(180, 152, 70, 60)
    with pytest.raises(ValueError, match="view 1"):                 # views that paste to different sizes
        CameraBatch(2, 200, 152, device="cpu", windowed=True).set([a, other])
    with pytest.raises(ValueError):
        CameraSlot.windowed(200, 152, device="cpu").set(other)
    bad = dict(a, crop=np.array([10, 10, 10, 10, a["width"] + 16, 152]))   # a window larger than the raster
    with pytest.raises(ValueError, match="does not fit"):
        crop_window(bad)
    pkg = {"means3D": torch.zeros(4, 3), "cov3D_precomp": torch.zeros(4, 6), "opacities": torch.zeros(4, 1), "shs": None,
           "rgb": torch.zeros(4, 3), "sh_degree": 0}
    with pytest.raises(ValueError, match="grad_sync"):
        render(a, pkg, torch.zeros(3), crop_window=True, grad_sync=object())
