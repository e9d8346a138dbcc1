"""Sample preparation on the GPU (d3ga_amd/sample_prep.py, csrc/sample_prep.hip) against the g++ build of csrc/sample_prep_math.h
(tests/sample_prep_ref.py: host_actorshq / host_goliath, itself held to the numpy oracle and the reference's loader by
tests/test_sample_prep_host.py): the kernels give its bytes for every output, both image dtypes and both store paths, at sizes
with odd row pitches (3 W bytes), windows larger than the image and rows that end on the last byte of their tensor.  Inputs are
tensors of exactly their size and outputs sit between guard bands.  Everything is integer or exactly representable: equality only."""
import ctypes

import numpy as np
import pytest
import torch

import sample_prep_ref as sr

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [(1, 1), (1, 5), (3, 1), (2, 3), (5, 7), (16, 64), (17, 63), (33, 65), (9, 260)]
GOLIATH_SIZES = [(2, 2), (7, 9), (64, 48), (5, 4)]
EXTRA = (2, 5)                                    # the part image is larger than the frame by this much
GUARD = 64                                        # bytes in front of and behind every output (keeps the 16-byte alignment)
FILL = 0xA5
NAMES = sr.NAMES
CAGES = {"body": {"label_id": [4]}, "upper": {"label_id": [1]}, "lower": {"label_id": [2, 3]}}


def _guarded(shape, dtype):
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    buf = torch.full((n + 2 * GUARD,), FILL, dtype=torch.uint8, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(dtype).view(shape)


def _bands_intact(buf):
    return bool((buf[:GUARD] == FILL).all()) and bool((buf[-GUARD:] == FILL).all())


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _src(t):
    """(pointer, pitch, frame) of a (B,H,W,...) uint8 tensor, as the Python layer derives them"""
    return ctypes.c_void_p(t.data_ptr()), t.stride(1), t.stride(0)


def _launch_actorshq(image, seg, mask, f32, outs, H, W):
    from d3ga_amd import _lib
    B = image.shape[0]
    path = ctypes.c_int32(-1)
    p = lambda n: None if outs[n] is None else ctypes.c_void_p(outs[n].data_ptr())
    _lib.check(_lib.lib().d3ga_sample_prep_actorshq(B, H, W, seg.shape[1], seg.shape[2], *_src(image), *_src(seg), *_src(mask), mask.stride(2) if W > 1 else 1,
                                                    int(f32), p("image"), p("seg_part"), p("seg_fg"), p("boundary_fg"), ctypes.byref(path),
                                                    _lib.stream_handle()), "d3ga_sample_prep_actorshq")
    torch.cuda.synchronize()
    return path.value


def _shapes(B, H, W, f32):
    return {"image": ((B, 3, H, W), torch.float32 if f32 else torch.uint8), "seg_part": ((B, 1, H, W), torch.int32),
            "seg_fg": ((B, 1, H, W), torch.float32), "boundary_fg": ((B, 1, H, W), torch.float32)}


@pytest.mark.parametrize("H,W", SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("B", [1, 3])
def test_kernel_bytes_equal_the_host_build(H, W, B):
    image, seg, mask = sr.random_actorshq(H * 1000 + W + B, B, H, W, EXTRA)
    t_image, t_seg, t_mask = _dev(image, seg, mask)
    assert t_image.numel() == B * H * W * 3 and t_seg.stride(1) == 3 * (W + EXTRA[1]) and t_image.stride(1) == 3 * W
    for f32 in (False, True):
        want, want_path = sr.host_actorshq(image, seg, mask, np.float32 if f32 else np.uint8)
        bufs = {n: _guarded(s, d) for n, (s, d) in _shapes(B, H, W, f32).items()}
        path = _launch_actorshq(t_image, t_seg, t_mask, f32, {n: v for n, (_, v) in bufs.items()}, H, W)
        assert path == want_path == int(W % 4 == 0)
        for n in NAMES:
            buf, view = bufs[n]
            assert _bands_intact(buf), (n, f32)
            got = view.cpu().numpy()
            assert got.dtype == want[n].dtype and np.array_equal(got, want[n]), (n, f32)


@pytest.mark.parametrize("H,W", [(5, 7), (16, 64), (9, 260)], ids=lambda v: str(v))
def test_views_are_addressed_in_place(H, W):
    """The matte as channel 0 of (B,H,W,3), a row-padded image, the part image cropped out of a larger buffer with its own pitch:
    the same bytes as from dense inputs.  The four-pixel path misaligned by one byte falls back to the other path, same bytes."""
    from d3ga_amd.sample_prep import prepare_actorshq
    B = 2
    image, seg, mask = sr.random_actorshq(H + W, B, H, W, EXTRA)
    want, _ = sr.host_actorshq(image, seg, mask)
    matte = np.random.default_rng(1).integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    matte[..., 0] = mask
    padded = np.full((B, H, W + 3, 3), 0xAB, np.uint8)
    padded[:, :, :W] = image
    big = np.full((B, H + 4, W + 9, 3), 0xCD, np.uint8)
    big[:, :H + EXTRA[0], :W + EXTRA[1]] = seg
    t_matte, t_padded, t_big = _dev(matte, padded, big)
    t_image, t_seg, t_mask = _dev(image, seg, mask)
    for args in ((t_image, t_seg, t_matte), (t_image, t_seg, t_matte[..., 0]), (t_padded[:, :, :W], t_seg, t_mask),
                 (t_image, t_big[:, :H + EXTRA[0], :W + EXTRA[1]], t_mask), (t_padded[:, :, :W], t_big[:, :H + 3, :W + 7], t_matte)):
        got = prepare_actorshq(*args)
        for n in NAMES:
            assert np.array_equal(got[n].cpu().numpy(), want[n]), n
    single = prepare_actorshq(t_image[1], t_seg[1], t_matte[1])                 # the 3-D forms, B = 1
    for n in NAMES:
        assert np.array_equal(single[n].cpu().numpy(), want[n][1:]), n
    # a uint8 image slot one byte off the 4-byte grid: the launch takes the one-pixel path and writes the same bytes
    buf, _ = _guarded((B * 3 * H * W + 1,), torch.uint8)
    slot = buf[GUARD + 1:GUARD + 1 + B * 3 * H * W].view(B, 3, H, W)
    outs = {"image": slot, "seg_part": None, "seg_fg": None, "boundary_fg": None}
    assert _launch_actorshq(t_image, t_seg, t_mask, False, outs, H, W) == 0
    assert np.array_equal(slot.cpu().numpy(), want["image"]) and bool((buf[:GUARD + 1] == FILL).all()) and bool((buf[-GUARD:] == FILL).all())


@pytest.mark.parametrize("skip", NAMES)
def test_outputs_are_skipped_one_at_a_time(skip):
    for (H, W) in ((5, 7), (4, 8)):
        B = 2
        image, seg, mask = sr.random_actorshq(77, B, H, W, EXTRA)
        want, _ = sr.host_actorshq(image, seg, mask, np.float32)
        bufs = {n: _guarded(s, d) for n, (s, d) in _shapes(B, H, W, True).items()}
        _launch_actorshq(*_dev(image, seg, mask), True, {n: (None if n == skip else v) for n, (_, v) in bufs.items()}, H, W)
        for n in NAMES:
            buf, view = bufs[n]
            if n == skip:                                     # an output passed as NULL: nothing anywhere near it is written
                assert bool((buf == FILL).all()), n
            else:
                assert _bands_intact(buf) and np.array_equal(view.cpu().numpy(), want[n]), n


def test_out_writes_in_place_and_allocates_nothing():
    from d3ga_amd.sample_prep import prepare_actorshq, prepare_goliath
    B, H, W = 2, 19, 36
    image, seg, mask = sr.random_actorshq(5, B, H, W, EXTRA)
    tensors = _dev(image, seg, mask)
    fresh = prepare_actorshq(*tensors, image_dtype=torch.float32)
    assert fresh["image"].dtype == torch.float32 and prepare_actorshq(*tensors)["image"].dtype == torch.uint8
    out = {n: torch.full(s, 99, dtype=d, device=DEV) for n, (s, d) in _shapes(B, H, W, True).items()}
    ptrs = {n: t.data_ptr() for n, t in out.items()}
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    res = prepare_actorshq(*tensors, out=out)
    assert torch.cuda.memory_allocated() == before
    for n in NAMES:
        assert res[n] is out[n] and out[n].data_ptr() == ptrs[n] and torch.equal(out[n], fresh[n]), n
    a = torch.zeros(B, 3, H, W, dtype=torch.uint8, device=DEV)                   # one slot only; its dtype decides
    res = prepare_actorshq(*tensors, image_dtype=torch.float32, out={"image": a})
    assert res["image"] is a and torch.equal(a.float(), fresh["image"]) and torch.equal(res["seg_part"], fresh["seg_part"])
    g_image, g_parts = _dev(*sr.random_goliath(6, B, H, W))
    fresh = prepare_goliath(g_image, g_parts)
    g_out = {n: torch.full((B, 3 if n == "image" else 1, H // 2, W // 2), float("nan"), device=DEV) for n in NAMES}
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    g_res = prepare_goliath(g_image, g_parts, out=g_out)
    assert torch.cuda.memory_allocated() == before
    for n in NAMES:
        assert g_res[n] is g_out[n] and torch.equal(g_out[n], fresh[n]), n


def test_graph_replay_follows_its_input_slots():
    from d3ga_amd.sample_prep import prepare_actorshq
    B, H, W = 1, 21, 44
    frames = [sr.random_actorshq(30 + i, B, H, W, EXTRA) for i in range(3)]
    eager = [prepare_actorshq(*_dev(*f)) for f in frames]
    slots = [torch.zeros_like(t) for t in _dev(*frames[0])]
    out = {n: torch.zeros(s, dtype=d, device=DEV) for n, (s, d) in _shapes(B, H, W, False).items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        prepare_actorshq(*slots, out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        prepare_actorshq(*slots, out=out)
    for i in (1, 0, 2):
        for slot, t in zip(slots, _dev(*frames[i])):
            slot.copy_(t)
        g.replay()
        torch.cuda.synchronize()
        for n in NAMES:
            assert torch.equal(out[n], eager[i][n]), (i, n)
    assert not torch.equal(eager[0]["seg_part"], eager[1]["seg_part"])


def test_sample_prep_equals_prepare_frames_fed_the_oracle():
    from d3ga_amd.frame_prep import FramePrep
    from d3ga_amd.sample_prep import SamplePrep
    cfg = {"train": {"erode_mask": True, "use_gamma_space": True}, "cages": CAGES}
    B, H, W = 2, 37, 70
    image, seg, mask = sr.random_actorshq(8, B, H, W, EXTRA)
    oracle = sr.actorshq_ref(image, seg, mask, np.float32)
    want = FramePrep(cfg)(*_dev(oracle["image"], oracle["seg_part"], oracle["seg_fg"]))
    prep = SamplePrep(cfg)
    got = prep.actorshq(*_dev(image, seg, mask))
    for n in ("image", "orig_image", "alpha", "silhouette"):
        assert torch.equal(got[n], want[n]), n
    for n in ("seg_fg", "boundary_fg", "seg_part"):
        assert np.array_equal(got[n].cpu().numpy(), oracle[n]) and got[n].dtype == (torch.int32 if n == "seg_part" else torch.float32), n
    assert 0.1 < float(got["alpha"].mean()) < 0.9 and bool((got["silhouette"][:, 0] != got["silhouette"][:, 1]).any())
    names = ("image", "orig_image", "alpha", "silhouette", "boundary_fg", "seg_fg")
    out = {n: torch.full_like(got[n], float("nan")) for n in names}
    res = prep.actorshq(*_dev(image, seg, mask), out=out)
    for n in names:
        assert res[n] is out[n] and torch.equal(out[n], got[n]), n
    # Goliath mode: the halved float frames, labels truncated by prepare_frames as .int() does
    g_image, g_parts = sr.random_goliath(9, B, H, W)
    g_parts[g_parts > 0] = g_parts[g_parts > 0] % 4 + 1
    oracle = sr.goliath_ref(g_image, g_parts)
    want = FramePrep(cfg)(*_dev(oracle["image"], oracle["seg_part"], oracle["seg_fg"]))
    got = prep.goliath(*_dev(g_image, g_parts))
    for n in ("image", "orig_image", "alpha", "silhouette"):
        assert torch.equal(got[n], want[n]), n
    for n in ("seg_fg", "boundary_fg", "seg_part"):
        assert np.array_equal(got[n].cpu().numpy(), oracle[n]), n


@pytest.mark.parametrize("H,W", GOLIATH_SIZES + [(3, 16), (9, 260)], ids=lambda v: str(v))
@pytest.mark.parametrize("B", [1, 3])
def test_goliath_kernel_bytes_equal_the_host_build(H, W, B):
    from d3ga_amd import _lib
    image, parts = sr.random_goliath(H * 100 + W + B, B, H, W)
    want, want_path = sr.host_goliath(image, parts)
    t_image, t_parts = _dev(image, parts)
    assert t_image.numel() == B * 3 * H * W
    for skip in (None,) + NAMES:
        bufs = {n: _guarded((B, 3 if n == "image" else 1, H // 2, W // 2), torch.float32) for n in NAMES}
        p = lambda n: None if n == skip else ctypes.c_void_p(bufs[n][1].data_ptr())
        path = ctypes.c_int32(-1)
        _lib.check(_lib.lib().d3ga_sample_prep_goliath(B, H, W, _lib.dptr(t_image), W, H * W, 3 * H * W, _lib.dptr(t_parts), W, H * W, p("image"),
                                                       p("seg_part"), p("seg_fg"), p("boundary_fg"), ctypes.byref(path), _lib.stream_handle()),
                   "d3ga_sample_prep_goliath")
        torch.cuda.synchronize()
        assert path.value == want_path == int((W // 2) % 4 == 0)
        for n in NAMES:
            buf, view = bufs[n]
            if n == skip:
                assert bool((buf == FILL).all()), n
            else:
                assert _bands_intact(buf) and np.array_equal(view.cpu().numpy(), want[n]), (n, skip)


def test_goliath_views_are_addressed_in_place():
    from d3ga_amd.sample_prep import prepare_goliath
    B, H, W = 2, 13, 22
    image, parts = sr.random_goliath(4, B, H + 1, W + 3)
    want, _ = sr.host_goliath(np.ascontiguousarray(image[:, :, 1:, 2:W + 2]), np.ascontiguousarray(parts[:, :, 1:, 2:W + 2]))
    t_image, t_parts = _dev(image, parts)
    got = prepare_goliath(t_image[:, :, 1:, 2:W + 2], t_parts[:, :, 1:, 2:W + 2])
    single = prepare_goliath(t_image[1, :, 1:, 2:W + 2], t_parts[1, :, 1:, 2:W + 2])
    for n in NAMES:
        assert np.array_equal(got[n].cpu().numpy(), want[n]) and np.array_equal(single[n].cpu().numpy(), want[n][1:]), n
