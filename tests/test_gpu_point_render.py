"""The point-cloud rasterizer and compositor on the GPU (d3ga_amd/point_render.py, csrc/point_raster.hip) against the float64
oracle (tests/point_ref.py), at the smallest shapes at which each mechanism can go wrong (point_ref.CASES): shell and solid
clouds of 3000 points at 70 x 90 and 90 x 70 (neither side a multiple of the 16-pixel tile), 6000 points whose busiest tile
list runs over three LDS batches, discs of 4 and 9 pixels in a 33 x 47 frame (boxes of up to 2 x 2 and 3 x 3 tiles), discs of
0.6 pixels (most miss every pixel centre), 200 points given twice (the tie rule), points behind the camera and outside the
frame, K = 1 and K = 8, P = 1, B = 3.  The tile table is built in workgroups of 256 tiles, so there are frames of exactly 256
tiles (a real tile's list ends at block_start[nblk]) and of 272, three views of 110 tiles (the table's workgroup boundary
inside a view), 257 views of one tile, and K = 2, 3, 4, 6, 7 for the other instantiations of the tile kernel;
test_a_quarter_million_one_pixel_views has 1025 table workgroups and more tiles than the tile kernel has workgroups.

idx equals the oracle's exactly away from the marginal pixels (a pixel centre within 1e-4 of a rim in dist2 / radius^2, or two
adjacent depths among the K + 1 nearest within 2e-6 z that do not belong to identical points; at most 3 % of the covered pixels
of a case, tests/test_point_render_host.py holds the cases to that); on a marginal pixel no chosen point lies beyond the rim by
more than 1e-4.  idx also equals the g++ build of csrc/point_raster_math.h bit for bit, everywhere.

Value bars, non-marginal pixels: 8 x the largest deviation of that g++ build (-ffp-contract=off) from the oracle over all cases,
as measured by tests/test_point_render_host.py (point_ref.MEASURED, point_ref.BARS):
                          measured    bar
  zbuf, relative          9.2e-8      7.36e-7
  dists / radius^2        1.8e-5      1.44e-4     (the worst: the 0.6-pixel discs, then the 256-pixel frames; 6.4e-6 otherwise)
  image                   1.7e-5      1.36e-4     (the worst: the 256-pixel frames)
The device build has contraction off and correctly rounded division, so it is expected to reproduce the host build to the
bit; the factor 8 is the issue's allowance.
"""
import ctypes

import numpy as np
import pytest
import torch

import point_ref as pr

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64                                        # words in front of and behind every output
NAN_BITS = 0x7FC0DEAD                             # a pattern no kernel would produce


def _setup_case(c):
    from d3ga_amd import MeshCameras
    cam = c["cams"].astype(np.float64)
    K = np.zeros((len(cam), 3, 3))
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = cam[:, 12], cam[:, 13], cam[:, 14], cam[:, 15], 1
    cams = MeshCameras(cam[:, :9].reshape(-1, 3, 3), cam[:, 9:12], K, (c["H"], c["W"]))
    assert np.array_equal(cams.data.cpu().numpy(), c["cams"])                 # the oracle and the device read the same 16 floats
    return cams, torch.from_numpy(c["points"]).to(DEV)


def _setup(ref):
    return _setup_case(ref.case)


def _renderer(ref, white=True):
    from d3ga_amd import PCRenderer
    r = PCRenderer(white_background=white, radius=ref.radius, points_per_pixel=ref.K)
    r.resize(ref.H, ref.W)
    return r


def _poisoned(scratch):
    """a scratch whose every byte is set: nothing in it may be assumed clean"""
    scratch.raw.fill_(0xFF)
    scratch.idx.fill_(12345)
    scratch.zbuf.fill_(float("nan"))
    scratch.dists.fill_(float("nan"))
    return scratch


def _np(*tensors):
    return [t.cpu().numpy() for t in tensors]


@pytest.mark.parametrize("name", pr.CASES)
def test_fragments_and_images_against_the_oracle_and_the_host_build(name):
    from d3ga_amd import rasterize_points
    ref = pr.reference(name)
    cams, verts = _setup(ref)
    r = _renderer(ref)
    scratch = _poisoned(r.scratch(cams, verts))
    frag = r.rasterize_points(cams, verts, scratch=scratch)
    assert frag.idx.shape == (ref.B, ref.H, ref.W, ref.K) and frag.idx.dtype == torch.int32
    assert frag.zbuf.shape == frag.dists.shape == frag.idx.shape and frag.zbuf.dtype == frag.dists.dtype == torch.float32
    idx, zbuf, dists = _np(*frag)
    dev = ref.check_fragments(idx, zbuf, dists)
    h_idx, h_zbuf, h_dists, _ = pr.host_fragments(ref.case)
    assert np.array_equal(idx, h_idx)                                          # the host build's idx, bit for bit
    print(f"{name}: zbuf equals the host build's: {np.array_equal(zbuf, h_zbuf)}, dists: {np.array_equal(dists, h_dists)}")
    free = rasterize_points(cams, verts, radius=ref.radius, points_per_pixel=ref.K)             # a fresh scratch, the module's function
    for a, b in zip(free, (idx, zbuf, dists)):
        assert np.array_equal(a.cpu().numpy(), b)
    colours = torch.from_numpy(ref.colours).to(DEV)
    dev["image"] = 0.0
    for white in (True, False):
        r = _renderer(ref, white)
        plain, coloured = r.render(cams, verts, scratch=_poisoned(scratch)), r.render(cams, verts, colours)
        assert plain.shape == (ref.B, ref.H, ref.W, 3) and plain.dtype == torch.float32
        dev["image"] = max(dev["image"], ref.check_image(plain.cpu().numpy(), white, False), ref.check_image(coloured.cpu().numpy(), white, True))
        assert torch.equal(r.forward(cams, verts), plain[0]) and torch.equal(r(cams, verts, colours), coloured[0])
        assert r(cams, verts).shape == (ref.H, ref.W, 3)
        if ref.B > 1:                                                          # one colour table for every cloud
            assert torch.equal(r.render(cams, verts, colours[0]), r.render(cams, verts, colours[:1].expand(ref.B, -1, -1).contiguous()))
    print(f"{name}: " + " ".join(f"{k} {v:.2e}" for k, v in sorted(dev.items())))
    for k, v in dev.items():
        assert v <= pr.BARS[k], (k, v, pr.BARS[k])
    if name == "one_point":
        assert int((idx[..., 0] == 0).sum()) == 21 and (idx[..., 1:] == -1).all()
    if name == "behind_and_outside":
        assert (idx < 1500).all()                                              # none of the 350 points behind the near plane


@pytest.mark.parametrize("name", ("shell_70x90", "dense6000", "duplicates", "tiles272"))
def test_two_runs_are_bit_identical_and_the_order_of_the_points_does_not_matter(name):
    ref = pr.reference(name)
    cams, verts = _setup(ref)
    r = _renderer(ref)
    colours = torch.from_numpy(ref.colours).to(DEV)
    first = [t.clone() for t in r.rasterize_points(cams, verts)] + [r.render(cams, verts, colours), r.render(cams, verts)]
    second = list(r.rasterize_points(cams, verts)) + [r.render(cams, verts, colours), r.render(cams, verts)]
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    back = verts.flip(1).contiguous()                                          # point p becomes point P - 1 - p
    frag = r.rasterize_points(cams, back)
    plain = r.render(cams, back)                                               # default colours: the same image
    if name != "duplicates":                                                   # (twins swap their slots: the smaller NEW index goes first)
        mapped = torch.where(frag.idx >= 0, ref.P - 1 - frag.idx, frag.idx)
        # two different points of one float32 depth in one pixel swap as twins do: such pixels (none, or next to none) are left out
        tie = ((frag.zbuf[..., 1:] == frag.zbuf[..., :-1]) & (frag.idx[..., 1:] >= 0)).any(-1)
        assert int(tie.sum()) <= 2 and torch.equal(frag.zbuf, first[1])
        assert torch.equal(mapped[~tie], first[0][~tie]) and torch.equal(frag.dists[~tie], first[2][~tie])
        assert torch.equal(r.render(cams, back, colours.flip(1).contiguous())[~tie], first[3][~tie]) and torch.equal(plain[~tie], first[4][~tie])
    else:
        assert torch.equal(frag.zbuf, first[1]) and torch.equal(frag.dists, first[2]) and torch.equal(plain, first[4])


@pytest.mark.parametrize("name", ("solid_90x70", "batch3"))
def test_a_captured_render_follows_its_vertices(name):
    ref = pr.reference(name)
    cams, verts = _setup(ref)
    r = _renderer(ref)
    colours = torch.from_numpy(ref.colours).to(DEV)
    moved = (verts * 0.9 + 0.02).contiguous()
    eager = [r.render(cams, v, colours) for v in (verts, moved)]
    assert not torch.equal(eager[0], eager[1])
    slot = verts.clone()
    scratch = _poisoned(r.scratch(cams, slot))
    out = torch.full_like(eager[0], float("nan"))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                             # warm-up outside the capture, as torch.cuda.graph asks
        assert r.render(cams, slot, colours, out=out, scratch=scratch) is out
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(out, eager[0])
    torch.cuda.set_sync_debug_mode("error")                   # nothing in the call waits for the device
    try:
        r.render(cams, slot, colours, out=out, scratch=scratch)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                             # one linear chain of launches
        r.render(cams, slot, colours, out=out, scratch=scratch)
    slot.copy_(moved)                                         # new vertex values, written in place
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager[1])
    with pytest.raises(ValueError):
        r.render(cams, slot[:, :-1], scratch=scratch)
    with pytest.raises(ValueError):
        r.render(cams, slot, out=out[..., :2])


def test_every_element_of_a_batch_is_its_own_single_call_and_grad_inputs_are_detached():
    from d3ga_amd import MeshCameras
    # views3_330: the tiles of view 2 lie on both sides of tile 256, where the second workgroup of the tile table begins
    for name in ("views3_330", "batch3"):
        ref = pr.reference(name)
        cams, verts = _setup(ref)
        r = _renderer(ref)
        frag = [t.clone() for t in r.rasterize_points(cams, verts)]
        image = r.render(cams, verts)
        assert not torch.equal(frag[0][0], frag[0][1])
        for b in range(ref.B):
            row = cams.data[b].double().cpu().numpy()
            K = np.array([[row[12], 0, row[14]], [0, row[13], row[15]], [0, 0, 1]])
            one = MeshCameras(row[:9].reshape(3, 3), row[9:12], K, (ref.H, ref.W))
            for a, w in zip(r.rasterize_points(one, verts[b:b + 1]), frag):
                assert torch.equal(a[0], w[b])
            assert torch.equal(r(one, verts[b:b + 1]), image[b])
    leaf = verts.clone().requires_grad_(True)
    got = r.render(cams, leaf)
    assert not got.requires_grad and torch.equal(got, image)


def test_raw_entry_points_stay_inside_their_buffers_and_an_empty_cloud_is_background():
    """Every output between guard bands, every element written; odd sizes, several workgroups; zbuf and dists optional."""
    from d3ga_amd import _lib
    L = _lib.lib()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    for name in ("batch3", "wider_discs", "solid_70x90", "tiles272", "views3_330"):      # the last two: two workgroups of the tile table
        ref = pr.reference(name)
        cams, verts = _setup(ref)
        B, P, H, W, K, radius = ref.B, ref.P, ref.H, ref.W, ref.K, ref.radius
        n = ctypes.c_size_t()
        assert L.d3ga_points_raster_scratch_bytes(B, P, H, W, radius, ctypes.byref(n)) == 0
        bufs = {}

        def guarded(key, shape, dtype=torch.float32):
            count = int(np.prod(shape))
            raw = torch.full((count + 2 * GUARD,), NAN_BITS, dtype=torch.int32, device=DEV)
            bufs[key] = raw
            return raw[GUARD:GUARD + count].view(dtype).view(shape)

        scratch = guarded("scratch", ((n.value + 3) // 4,), torch.int32)
        idx, zbuf, dists = guarded("idx", (B, H, W, K), torch.int32), guarded("zbuf", (B, H, W, K)), guarded("dists", (B, H, W, K))
        image = guarded("image", (B, H, W, 3))
        s = _lib.stream_handle()
        bg = (ctypes.c_float * 3)(1, 1, 1)
        assert L.d3ga_points_rasterize(B, P, H, W, K, radius, p(verts), p(cams.data), p(scratch), p(idx), p(zbuf), p(dists), s) == 0
        assert L.d3ga_points_composite(B, P, H, W, K, radius, p(idx), p(dists), None, bg, p(image), s) == 0
        torch.cuda.synchronize()
        for key, raw in bufs.items():
            assert (raw[:GUARD] == NAN_BITS).all() and (raw[-GUARD:] == NAN_BITS).all(), (name, key)
            if key != "scratch":
                assert not (raw[GUARD:-GUARD] == NAN_BITS).any(), (name, key)
        ref.check_fragments(*_np(idx, zbuf, dists))
        idx2 = guarded("idx2", (B, H, W, K), torch.int32)
        assert L.d3ga_points_rasterize(B, P, H, W, K, radius, p(verts), p(cams.data), p(scratch), p(idx2), None, None, s) == 0
        torch.cuda.synchronize()
        assert torch.equal(idx2, idx) and (bufs["idx2"][:GUARD] == NAN_BITS).all() and (bufs["idx2"][-GUARD:] == NAN_BITS).all()
    from d3ga_amd import PCRenderer
    ref = pr.reference("shell_70x90")
    cams, verts = _setup(ref)
    for white in (True, False):
        r = PCRenderer(white_background=white)
        frag = r.rasterize_points(cams, verts[:, :0])
        assert (frag.idx == -1).all() and (frag.zbuf == -1).all() and (frag.dists == -1).all()
        assert (r.render(cams, verts[:, :0]) == (1.0 if white else 0.0)).all()


def test_a_quarter_million_one_pixel_views():
    """The tile table beyond one trip of its scan kernel, and more tiles than the tile kernel has workgroups.
    pixels262400: 262 400 views of a 1 x 1 frame, 4 points each: 1025 table workgroups (points_scan_kernel makes a second trip
    and carries the first trip's total into it) and 262 400 tiles for 65 536 tile workgroups (four trips, a fifth for 256 of
    them).  idx equals the host build's in every view; every 997th view (264) is held to the float64 oracle.
    views257_k1: 257 views of 256 x 256 with 200 points each, K = 1, through the raw entry point without zbuf and dists: 65 792
    tiles, so the first 256 tile workgroups make a second trip, on the tiles of the last view."""
    from d3ga_amd import _lib, rasterize_points
    c, h_idx, h_zbuf, h_dists = pr.big_case("pixels262400")
    cams, verts = _setup_case(c)
    B, K = len(c["points"]), c["K"]
    assert pr.n_tiles(c) == B == 1025 * pr.TABLE_BLOCK > 4 * 65536
    idx, zbuf, dists = _np(*rasterize_points(cams, verts, radius=c["radius"], points_per_pixel=K))
    assert idx.shape == (B, 1, 1, K)
    wrong = np.flatnonzero((idx != h_idx).any(axis=(1, 2, 3)))
    assert not len(wrong), f"{len(wrong)} views with other points than the host build's, the first is view {wrong[0]} (table workgroup {wrong[0] // 256})"
    covered = float((idx[..., 0] >= 0).mean())
    assert 0.25 <= covered <= 0.75
    filled = idx >= 0
    assert (zbuf[~filled] == -1).all() and (dists[~filled] == -1).all()
    dev = {"zbuf_rel": float((np.abs(zbuf[filled].astype(np.float64) - h_zbuf[filled]) / h_zbuf[filled]).max()),
           "dists": float(np.abs(dists[filled].astype(np.float64) - h_dists[filled]).max()) / c["radius"] ** 2}
    print(f"pixels262400: {covered * 100:.1f} % of the views covered; against the host build: " + " ".join(f"{k} {v:.2e}" for k, v in sorted(dev.items())))
    for k, v in dev.items():
        assert v <= pr.BARS[k], (k, v, pr.BARS[k])
    views, ref = pr.sampled_reference("pixels262400", 997)
    dev = ref.check_fragments(idx[views], zbuf[views], dists[views])
    print(f"pixels262400[::997]: against the oracle: " + " ".join(f"{k} {v:.2e}" for k, v in sorted(dev.items())))
    for k, v in dev.items():
        assert v <= pr.BARS[k], (k, v, pr.BARS[k])
    del idx, zbuf, dists

    c, h_idx, _, _ = pr.big_case("views257_k1", values=False)
    cams, verts = _setup_case(c)
    B, P, H, W, K, radius = len(c["points"]), c["points"].shape[1], c["H"], c["W"], c["K"], c["radius"]
    assert pr.n_tiles(c) == 65536 + 256 and K == 1
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    n = ctypes.c_size_t()
    assert L.d3ga_points_raster_scratch_bytes(B, P, H, W, radius, ctypes.byref(n)) == 0
    scratch = torch.full(((n.value + 3) // 4 + 2 * GUARD,), NAN_BITS, dtype=torch.int32, device=DEV)
    raw = torch.full((B * H * W * K + 2 * GUARD,), NAN_BITS, dtype=torch.int32, device=DEV)
    assert L.d3ga_points_rasterize(B, P, H, W, K, radius, p(verts), p(cams.data), p(scratch[GUARD:]), p(raw[GUARD:]), None, None,
                                   _lib.stream_handle()) == 0
    torch.cuda.synchronize()
    for band in (raw[:GUARD], raw[-GUARD:], scratch[:GUARD], scratch[-GUARD:]):
        assert (band == NAN_BITS).all()
    idx = raw[GUARD:-GUARD].view(B, H, W, K).cpu().numpy()
    wrong = np.flatnonzero((idx != h_idx).any(axis=(1, 2, 3)))
    assert not len(wrong), f"{len(wrong)} views with other points than the host build's, the first is view {wrong[0]}"
    print(f"views257_k1: idx equals the host build's in all {B} views, {int((idx[-1] >= 0).sum())} covered pixels in the last")
