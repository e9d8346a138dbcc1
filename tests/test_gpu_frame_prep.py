"""Frame preparation on the GPU (d3ga_amd/frame_prep.py, csrc/frame_prep.hip) against the numpy oracle (tests/frame_ref.py):
every flag that changes a path, at the shapes where a tile (64 x 32), a halo or a 16-byte quad changes, between guard bands.
Masks, silhouette and the fg selection of `image` are exact on every pixel; colour is within the derived 1e-6 bar."""
import ctypes

import numpy as np
import pytest
import torch

import frame_ref as fr

pytestmark = pytest.mark.gpu
DEV = "cuda"
GAMMA, BG_WHITE, ERODE_MASK, CLOSE_HOLES, IMAGE_U8, SEG_F32 = 1, 2, 4, 8, 16, 32
COLOR_BAR = 1e-6                                  # derived in tests/test_frame_prep_host.py
GUARD = 64                                        # floats in front of and behind every output (keeps the 16-byte alignment)
NAN_BITS = 0x7FC0DEAD                             # a NaN pattern no kernel would produce
GOLIATH = {"body": {"label_id": [1]}, "upper": {"label_id": [27]}, "lower": {"label_id": [16]}}
NAMES = ("image", "orig_image", "alpha", "silhouette")

# (H, W, B, flags, seg_fg given, outputs passed as NULL).  W in {1, 5, 63, 64, 65, 130} x H in {1, 3, 17, 33, 70} pairwise; W = 65
# with B = 2 starts rows off the 16-byte grid; every flag appears set and clear, the four morphology combinations, both image
# and label types, seg_fg NULL, B = 3
CASES = [
    (1, 1, 1, 0, True, ()),
    (3, 5, 1, GAMMA | BG_WHITE | ERODE_MASK, True, ()),
    (17, 63, 1, CLOSE_HOLES | IMAGE_U8, True, ()),
    (33, 64, 1, GAMMA | BG_WHITE | ERODE_MASK | CLOSE_HOLES | SEG_F32, True, ()),
    (3, 65, 2, BG_WHITE | ERODE_MASK, True, ()),
    (70, 130, 1, GAMMA | BG_WHITE | CLOSE_HOLES | IMAGE_U8 | SEG_F32, True, ()),
    (33, 5, 3, ERODE_MASK | CLOSE_HOLES, True, ()),
    (70, 65, 2, GAMMA | BG_WHITE | ERODE_MASK | CLOSE_HOLES, False, ()),
    (17, 130, 1, GAMMA, True, ("image", "alpha")),
    (33, 1, 1, BG_WHITE | IMAGE_U8 | ERODE_MASK | CLOSE_HOLES, False, ()),
    (1, 63, 1, GAMMA | BG_WHITE | CLOSE_HOLES, True, ("orig_image", "silhouette")),
    (17, 64, 1, IMAGE_U8 | SEG_F32, False, ("image", "orig_image", "silhouette")),
]


def _inputs(seed, B, H, W, float_labels):
    rng = np.random.default_rng(seed)
    image = rng.integers(0, 256, (B, 3, H, W)).astype(np.float32)
    image.reshape(-1)[:9] = np.arange(9)[: image.size]        # where the black clamp bites
    # blocks of 6 x 6 pixels switched on or off, 8 % of the pixels flipped: shapes the median and the morphology really change
    coarse = rng.random((B, 1, H // 6 + 1, W // 6 + 1)) < 0.5
    mask = np.kron(coarse, np.ones((6, 6), dtype=bool))[:, :, :H, :W] ^ (rng.random((B, 1, H, W)) < 0.08)
    seg = np.where(mask, rng.integers(1, 30, (B, 1, H, W)), 0).astype(np.float32)
    flat = seg.reshape(-1)
    special = [-3.0, 77.0] + ([0.5, 26.9, -0.5, 27.5, 16.2] if float_labels else [])     # negative, behind the table, fractions
    flat[rng.choice(flat.size, min(len(special), flat.size), replace=False)] = special[: flat.size]
    seg_fg = (mask & (rng.random((B, 1, H, W)) < 0.5)).astype(np.float32)
    seg_fg.reshape(-1)[rng.integers(0, seg_fg.size, 3)] = 1.0     # foreground by seg_fg alone
    return image, seg, seg_fg


def _guarded(shape):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), NAN_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _bands_intact(buf, n):
    bits = buf.view(torch.int32)
    return bool((bits[:GUARD] == NAN_BITS).all()) and bool((bits[GUARD + n:] == NAN_BITS).all())


@pytest.mark.parametrize("H,W,B,flags,with_fg,null", CASES, ids=lambda v: str(v) if not isinstance(v, tuple) else "-".join(v) or "all")
def test_every_path_against_the_oracle(H, W, B, flags, with_fg, null):
    from d3ga_amd import _lib
    from d3ga_amd.frame_prep import silhouette_table
    image, seg, seg_fg = _inputs(H * 1000 + W + flags, B, H, W, bool(flags & SEG_F32))
    bgname = "white" if flags & BG_WHITE else "black"
    table, other, _ = silhouette_table(GOLIATH, bgname, device=DEV)
    t_img = torch.from_numpy(image.astype(np.uint8) if flags & IMAGE_U8 else image).to(DEV)
    t_seg = torch.from_numpy(seg if flags & SEG_F32 else seg.astype(np.int32)).to(DEV)
    t_fg = torch.from_numpy(seg_fg).to(DEV) if with_fg else None
    bufs = {n: _guarded((B, 1 if n == "alpha" else 3, H, W)) for n in NAMES}
    p = lambda n: None if n in null else ctypes.c_void_p(bufs[n][1].data_ptr())
    _lib.check(_lib.lib().d3ga_frame_prep(B, H, W, flags, _lib.dptr(t_img), _lib.dptr(t_seg), _lib.dptr(t_fg), _lib.dptr(table), table.shape[0],
                                          _lib.dptr(other), p("image"), p("orig_image"), p("alpha"), p("silhouette"), _lib.stream_handle()),
               "d3ga_frame_prep")
    torch.cuda.synchronize()
    want = fr.frame_ref(image, seg if flags & SEG_F32 else seg.astype(np.int32), seg_fg if with_fg else None, GOLIATH, bool(flags & GAMMA),
                        bgname, bool(flags & ERODE_MASK), bool(flags & CLOSE_HOLES))
    got = {}
    for n in NAMES:
        buf, view = bufs[n]
        if n in null:                                         # an output passed as NULL: nothing anywhere near it is written
            assert bool((buf.view(torch.int32) == NAN_BITS).all()), n
            continue
        assert _bands_intact(buf, view.numel()), n
        got[n] = view.cpu().numpy()
        assert np.isfinite(got[n]).all(), n                   # every pixel was written
    if "alpha" in got:
        assert np.array_equal(got["alpha"], want["alpha"])
    if "silhouette" in got:
        assert np.array_equal(got["silhouette"], want["silhouette"])
    if "orig_image" in got:
        err = float(np.abs(got["orig_image"] - want["orig_image"]).max())
        print(f"orig_image: worst |a - b| = {err:.3e} = {err / COLOR_BAR:.3f} of the bar")
        assert err <= COLOR_BAR
    if "image" in got:
        bgv = np.float32(1.0 if flags & BG_WHITE else 0.0)
        if "orig_image" in got:                               # the fg selection: exact, on every pixel
            assert np.array_equal(got["image"], np.where(want["fg"], got["orig_image"], bgv))
        assert float(np.abs(got["image"] - want["image"]).max()) <= COLOR_BAR


def test_labels_truncate_and_fall_back_to_the_other_colour():
    from d3ga_amd.frame_prep import silhouette_table, prepare_frames
    vals = [0.5, 26.9, -0.5, 27.0, 27.9, 16.0, -1.0, -7.3, 28.0, 1e6, 0.0, 1.2]
    seg = torch.tensor(vals, device=DEV).view(1, 1, 1, len(vals))
    img = torch.zeros(1, 3, 1, len(vals), device=DEV)
    table = silhouette_table(GOLIATH, "black", device=DEV)
    for s in (seg, seg.int()):                                # the float path and .int() on the host agree
        out = prepare_frames(img, s, None, table=table, gamma=False, background="black")
        sil = out["silhouette"][0, :, 0].t().cpu().tolist()
        black, red, green, blue = [0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]
        assert sil == [black, blue, black, red, red, green, blue, blue, blue, blue, black, blue], sil
    assert out["seg_fg"] is None


def test_out_writes_in_place_and_allocates_nothing():
    from d3ga_amd.frame_prep import FramePrep
    B, H, W = 2, 37, 70
    image, seg, seg_fg = _inputs(5, B, H, W, False)
    prep = FramePrep({"train": {"erode_mask": True, "use_gamma_space": True}, "cages": GOLIATH})
    t_img, t_seg, t_fg = torch.from_numpy(image).to(DEV), torch.from_numpy(seg.astype(np.int32)).to(DEV), torch.from_numpy(seg_fg).to(DEV)
    fresh = prep(t_img, t_seg, t_fg)
    out = {n: torch.full((B, 1 if n == "alpha" else 3, H, W), float("nan"), device=DEV) for n in NAMES}
    ptrs = {n: t.data_ptr() for n, t in out.items()}
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    res = prep(t_img, t_seg, t_fg, out=out)
    assert torch.cuda.memory_allocated() == before
    torch.cuda.synchronize()
    for n in NAMES:
        assert res[n] is out[n] and out[n].data_ptr() == ptrs[n]
        assert torch.equal(out[n], fresh[n]), n
    assert res["seg_fg"] is t_fg
    want = fr.frame_ref(image, seg.astype(np.int32), seg_fg, GOLIATH, True, "white", True, False)
    assert np.array_equal(out["alpha"].cpu().numpy(), want["alpha"])
    # one slot only: the others are allocated, the given one is written
    a = torch.zeros(B, 1, H, W, device=DEV)
    res = prep(t_img, t_seg, t_fg, out={"alpha": a})
    assert res["alpha"] is a and torch.equal(a, fresh["alpha"]) and torch.equal(res["image"], fresh["image"])
    # a uint8 image gives the same frames bit for bit
    res8 = prep(t_img.to(torch.uint8), t_seg, t_fg)
    for n in NAMES:
        assert torch.equal(res8[n], fresh[n]), n


def test_captured_step_follows_its_input_slots():
    from d3ga_amd.frame_prep import FramePrep
    from d3ga_amd.graph import CapturedStep
    B, H, W = 1, 45, 67
    prep = FramePrep({"train": {"use_close_holes": True, "use_gamma_space": True, "background": "black"}, "cages": GOLIATH})
    frames = [_inputs(20 + i, B, H, W, False) for i in range(3)]
    dev = lambda f: (torch.from_numpy(f[0]).to(DEV), torch.from_numpy(f[1].astype(np.int32)).to(DEV), torch.from_numpy(f[2]).to(DEV))
    eager = [prep(*dev(f)) for f in frames]
    slots = dict(zip(("image", "seg_part", "seg_fg"), (torch.zeros_like(t) for t in dev(frames[0]))))
    out = {n: torch.zeros(B, 1 if n == "alpha" else 3, H, W, device=DEV) for n in NAMES}
    cap = CapturedStep(lambda: prep(slots["image"], slots["seg_part"], slots["seg_fg"], out=out), slots=slots)
    for i in (1, 0, 2):
        img, seg, sfg = dev(frames[i])
        res = cap.replay(image=img, seg_part=seg, seg_fg=sfg)
        torch.cuda.synchronize()
        for n in NAMES:
            assert res[n] is out[n] and torch.equal(out[n], eager[i][n]), (i, n)
    assert not torch.equal(eager[0]["alpha"], eager[1]["alpha"])
