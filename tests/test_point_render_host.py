"""The point-cloud rasterizer and compositor without a GPU.  pytorch3d cannot be run next to this library, so no golden exists:
the float64 oracle (tests/point_ref.py, written from DESIGN.md 4.4h) is checked from first principles instead (hand-computed
single points, ties, stacks, the near plane, the frame's edge, both aspect ratios), and the g++ build of
csrc/point_raster_math.h -- the text the kernels run, at -ffp-contract=off as the device build -- is held to the oracle: idx
exactly away from the marginal pixels, the values within an eighth of the bars of the GPU tests (point_ref.BARS, which are 8 x
what this module measures).  Then the marginal cap, the ABI surface, its refusals and the Python layer's ValueErrors."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import point_ref as pr
from conftest import ROOT

E_NULL, E_SIZE, E_CONFIG = -1, -2, -3            # D3GA_E_* (include/d3ga.h)
NEW_EXPORTS = ("d3ga_points_raster_scratch_bytes", "d3ga_points_rasterize", "d3ga_points_composite")


def _ident(H, W, f=10.0, cx=None, cy=None):
    return pr.cam_row(np.eye(3), np.zeros(3), f, f, 0.5 * W if cx is None else cx, 0.5 * H if cy is None else cy)


def _at(cam, u, v, z):
    """the world point (camera at the origin, no rotation) that projects to (u, v) at depth z"""
    fx, fy, cx, cy = (float(c) for c in cam[12:16])
    return [(u - cx) / fx * z, (v - cy) / fy * z, z]


def _both(points, cam, H, W, r_px, K):
    """oracle and host build of one hand-made cloud -> (oracle dict, host idx, host zbuf, host dists, case)"""
    case = pr._one(np.asarray(points, np.float32), cam, H, W, r_px, K)
    ref = pr.rasterize_ref(case["points"][0], case["cams"][0], H, W, case["radius"], K)
    idx, zbuf, dists, _ = pr.host_fragments(case)
    return ref, idx[0], zbuf[0], dists[0], case


# ---- the oracle (and the host build) from first principles ------------------------------------------------------------------
def test_a_point_at_a_pixel_centre_gives_exactly_its_colour():
    H, W = 12, 16                                             # min = 12, r_px = 2.5: radius = 5 / 12
    cam = _ident(H, W)
    ref, idx, zbuf, dists, case = _both([_at(cam, 5.5, 3.5, 2.0)], cam, H, W, 2.5, 5)
    colour = np.array([[0.25, 0.5, 0.75]], np.float32)
    for got_idx, got_d in ((ref["idx"], ref["dists"]), (idx, dists)):
        assert got_idx[3, 5, 0] == 0 and (got_idx[3, 5, 1:] == -1).all() and abs(float(got_d[3, 5, 0])) <= 1e-12
        img = pr.composite_ref(np.asarray(got_idx, np.int64), np.asarray(got_d, np.float64), case["radius"], colour, white=True)
        assert np.array_equal(img[3, 5], colour[0].astype(np.float64))                          # w = 1: the colour itself
    # the pixels of the disc: centres within 2.5 px of (5.5, 3.5): dx^2 + dy^2 < 6.25 for integer dx, dy: 21 pixels
    want = np.array([[(i - 5) ** 2 + (j - 3) ** 2 < 6.25 for i in range(W)] for j in range(H)])
    assert np.array_equal(ref["covered"], want) and int(want.sum()) == 21 and np.array_equal(idx[..., 0] >= 0, want)
    assert float(ref["zbuf"][3, 5, 0]) == 2.0 and float(zbuf[3, 5, 0]) == 2.0
    image = pr.host_image(case, idx[None], dists[None], colour[None], True)[0]
    assert np.array_equal(image[3, 5], colour[0]) and (image[~want] == 1).all()
    assert (pr.host_image(case, idx[None], dists[None], None, False)[0][~want] == 0).all()


def test_a_point_at_distance_d_is_weighted_without_the_background():
    H, W = 12, 16
    cam = _ident(H, W)
    ref, idx, zbuf, dists, case = _both([_at(cam, 5.5, 3.5, 2.0)], cam, H, W, 2.5, 5)
    # pixel (7, 4): d^2 = 2^2 + 1^2 = 5 px^2, w = 1 - 5 / 6.25 = 0.2; dist2 in NDC units = 5 (2 / 12)^2
    assert abs(float(ref["dists"][4, 7, 0]) - 5 * (2 / 12) ** 2) <= 1e-12
    for white in (True, False):
        img = pr.composite_ref(ref["idx"], ref["dists"], case["radius"], None, white)
        assert float(np.abs(img[4, 7] - 0.2 * pr.DEFAULT_COLOR).max()) <= 1e-6                  # radius is a float32 value
        got = pr.host_image(case, idx[None], dists[None], None, white)[0]
        assert float(np.abs(got[4, 7] - 0.2 * pr.DEFAULT_COLOR).max()) <= 1e-6
    assert float(np.abs(pr.DEFAULT_COLOR * 255 - [154, 205, 50]).max()) <= 1e-12


def test_two_fragments_composite_front_to_back():
    H, W = 12, 16
    cam = _ident(H, W)
    ref, idx, _, dists, case = _both([_at(cam, 5.5, 3.5, 3.0), _at(cam, 6.5, 3.5, 2.0)], cam, H, W, 2.5, 5)
    assert ref["idx"][3, 5, :3].tolist() == [1, 0, -1] and idx[3, 5, :3].tolist() == [1, 0, -1]       # the nearer first
    colours = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], np.float32)
    w_front, w_back = 1 - 1 / 6.25, 1.0                       # the front point is 1 px away, the back one at the centre
    want = np.array([w_back * (1 - w_front), w_front, 0.0])
    img = pr.composite_ref(ref["idx"], ref["dists"], case["radius"], colours, True)
    assert float(np.abs(img[3, 5] - want).max()) <= 1e-7
    assert float(np.abs(pr.host_image(case, idx[None], dists[None], colours[None], True)[0][3, 5] - want).max()) <= 1e-6


def test_coincident_points_fill_slots_in_index_order_and_stacks_keep_the_nearest():
    H, W = 12, 16
    cam = _ident(H, W)
    p = _at(cam, 5.5, 3.5, 2.0)
    ref, idx, _, _, _ = _both([p, _at(cam, 9.5, 8.5, 2.5), p, p], cam, H, W, 2.5, 3)
    assert ref["idx"][3, 5].tolist() == [0, 2, 3] and idx[3, 5].tolist() == [0, 2, 3] and not ref["marginal"][3, 5]
    K = 3                                                     # K + 2 stacked points, given far to near: the K nearest, nearest first
    stack = [_at(cam, 5.5, 3.5, z) for z in (3.0, 2.8, 2.6, 2.4, 2.2)]
    ref, idx, zbuf, _, _ = _both(stack, cam, H, W, 2.5, K)
    assert ref["idx"][3, 5].tolist() == [4, 3, 2] and idx[3, 5].tolist() == [4, 3, 2]
    assert np.allclose(zbuf[3, 5], [2.2, 2.4, 2.6], rtol=1e-6) and int(ref["members"][3, 5]) == 5


def test_the_near_plane_drops_and_the_frame_edge_does_not():
    H, W = 12, 16
    cam = _ident(H, W)
    ref, idx, _, _, _ = _both([_at(cam, 5.5, 3.5, 0.005), _at(cam, 5.5, 3.5, -1.0)], cam, H, W, 2.5, 5)
    assert (ref["idx"] == -1).all() and (idx == -1).all()
    # a centre 1.2 px left of the frame: the disc reaches three pixel centres of column 0 (1.7 px away in its own row) and none of column 1
    ref, idx, _, _, _ = _both([_at(cam, -1.2, 3.5, 2.0)], cam, H, W, 2.5, 5)
    want = np.zeros((H, W), bool)
    for j in range(H):
        for i in range(W):
            want[j, i] = (i + 0.5 + 1.2) ** 2 + (j - 3) ** 2 < 6.25
    assert want.sum() == 3 and np.array_equal(ref["covered"], want) and np.array_equal(idx[..., 0] >= 0, want)


def test_the_radius_is_measured_on_the_shorter_side():
    for H, W in ((12, 40), (40, 12)):
        cam = _ident(H, W)
        radius = 0.45                                         # r_px = 0.45 * 12 / 2 = 2.7 whichever side is the shorter
        case = dict(points=np.array([[_at(cam, 6.5, 6.5, 2.0)]], np.float32), cams=cam[None], H=H, W=W, radius=radius, K=2)
        ref = pr.rasterize_ref(case["points"][0], cam, H, W, radius, 2)
        want = np.array([[(i - 6) ** 2 + (j - 6) ** 2 < 7.29 for i in range(W)] for j in range(H)])
        assert np.array_equal(ref["covered"], want) and want.sum() == 21
        idx, _, dists, _ = pr.host_fragments(case)
        assert np.array_equal(idx[0, ..., 0] >= 0, want)
        assert abs(float(dists[0, 6, 8, 0]) - 4 * (2 / 12) ** 2) <= 1e-7 and abs(float(ref["dists"][6, 8, 0]) - 4 / 36) <= 1e-7      # the point's float32 coordinates are not exact here


# ---- the host build against the oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pr.CASES)
def test_marginal_pixels_stay_under_the_cap(name):
    ref = pr.reference(name)
    share, covered = ref.marginal_share()
    print(f"{name}: {share * 100:.2f} % of {covered} covered pixels are marginal, up to {max(int(f['members'].max()) for f in ref.frag)} members per pixel")
    assert covered > 0 and share <= pr.MARGINAL_CAP


@pytest.mark.parametrize("name", pr.CASES)
def test_host_build_equals_the_oracle(name):
    ref = pr.reference(name)
    c = ref.case
    idx, zbuf, dists, longest = pr.host_fragments(c)
    dev = ref.check_fragments(idx, zbuf, dists)
    dev["image"] = 0.0
    for white in (True, False):
        for coloured in (False, True):
            image = pr.host_image(c, idx, dists, ref.colours if coloured else None, white)
            dev["image"] = max(dev["image"], ref.check_image(image, white, coloured))
    print(f"{name}: longest tile list {longest} " + " ".join(f"{k} {v:.2e}" for k, v in sorted(dev.items())))
    for k, v in dev.items():
        assert 8 * v <= pr.BARS[k], (k, v)
    # the box loses no member, and the order in which the lists are filled changes nothing
    lib = pr.host_lib()
    args = (ref.B, ref.P, ref.H, ref.W, ctypes.c_float(ref.radius), pr._ptr(np.ascontiguousarray(c["points"])), pr._ptr(np.ascontiguousarray(c["cams"])))
    assert lib.hc_points_members_plain(*args) == lib.hc_points_members_tiled(*args)
    other = pr.host_fragments(c, reversed_lists=True)
    assert all(np.array_equal(a, b) for a, b in zip((idx, zbuf, dists), other[:3]))
    if name == "dense6000":
        assert longest > 3 * 256                              # more than three LDS batches of the tile kernel
    if name in ("wide_discs", "wider_discs"):                 # some box spans 2 (r_px = 4) or 3 (r_px = 9) tiles each way, in the oracle's own terms
        r_px, most = (4.0, 2) if name == "wide_discs" else (9.0, 3)
        u, v, z, keep = pr.project_ref(c["points"][0], c["cams"][0])
        span = lambda a, n: np.clip(np.floor(a + r_px - 0.5), 0, n - 1) // 16 - np.clip(np.ceil(a - r_px - 0.5), 0, n - 1) // 16 + 1
        assert span(u, ref.W)[keep].max() == most == span(v, ref.H)[keep].max()
    if name == "narrow_discs":
        assert sum(int(f["covered"].sum()) for f in ref.frag) < 0.6 * ref.P                    # most discs miss every pixel centre
    if name == "behind_and_outside":
        u, v, z, keep = pr.project_ref(c["points"][0], c["cams"][0])
        assert (~keep).sum() == 350 and ((u < -3) | (u > ref.W + 3))[keep].sum() > 100
    if name == "duplicates":                                  # both copies in adjacent slots, the smaller index first, and held exactly
        pts = c["points"][0]
        twins = 0
        f = ref.frag[0]
        a, b = f["idx"][..., :-1], f["idx"][..., 1:]
        pair = (a >= 0) & (b >= 0) & (pts[np.maximum(a, 0)] == pts[np.maximum(b, 0)]).all(-1)
        twins = int(pair.sum())
        assert twins > 200 and (a[pair] < b[pair]).all() and (pair.any(-1) & ~f["marginal"]).sum() > 100


def test_the_table_cases_have_the_tile_counts_they_are_named_for():
    """The tile table of csrc/point_raster.hip is built in workgroups of 256 tiles: one full workgroup, two, a boundary inside a
    view, a second workgroup of one tile; then more workgroups than one trip of its scan kernel and more tiles than the tile
    kernel has workgroups."""
    want = {"tiles256": 256, "tiles272": 272, "views3_330": 330, "views257": 257, "pixels262400": 262400, "views257_k1": 65792}
    for name, tiles in want.items():
        c = pr.make_case(name)
        assert pr.n_tiles(c) == tiles and (name in pr.CASES) == (tiles < 1000), name
    assert pr.TABLE_BLOCK == 256 and 262400 == 1025 * pr.TABLE_BLOCK and 65792 == 65536 + 256
    assert sorted(pr.make_case(n)["K"] for n in pr.CASES if n[0] == "k" or n == "solid_70x90") == list(range(1, 9))       # every points_tile_kernel<K>


def test_the_one_pixel_views_are_half_covered_and_the_host_build_equals_the_oracle_on_every_997th():
    c, idx, zbuf, dists = pr.big_case("pixels262400")
    assert idx.shape == (262400, 1, 1, 5) and c["points"].shape == (262400, 4, 3)
    covered = float((idx[..., 0] >= 0).mean())
    print(f"pixels262400: {covered * 100:.1f} % of the views covered, {float((idx[..., 1] >= 0).mean()) * 100:.1f} % by two points or more")
    assert 0.25 <= covered <= 0.75
    assert (idx[..., 4] == -1).all() and (idx[..., 3] >= 0).any()                          # P = 4: slot 4 stays empty, slot 3 does not
    views, ref = pr.sampled_reference("pixels262400", 997)
    assert len(views) == 264 and views[-1] == 262211
    share, n = ref.marginal_share()
    dev = ref.check_fragments(idx[views], zbuf[views], dists[views])
    print(f"pixels262400[::997]: {share * 100:.2f} % of {n} covered pixels are marginal " + " ".join(f"{k} {v:.2e}" for k, v in sorted(dev.items())))
    assert 0.25 * len(views) <= n <= 0.75 * len(views) and share <= pr.MARGINAL_CAP
    for k, v in dev.items():
        assert 8 * v <= pr.BARS[k], (k, v)


def test_the_second_trip_of_the_tile_kernel_meets_covered_tiles():
    """views257_k1: the tiles past 65 536 are the last view's; its pixels must not all be background."""
    c, idx, _, _ = pr.big_case("views257_k1", values=False)
    assert idx.shape == (257, 256, 256, 1) and ((idx >= -1) & (idx < 200)).all()
    per_view = (idx[..., 0] >= 0).reshape(257, -1).sum(1)
    print(f"views257_k1: {int(per_view.min())} .. {int(per_view.max())} covered pixels per view, {int(per_view[-1])} in the last")
    assert per_view.min() > 500
    tiles = (idx[-1, ..., 0] >= 0).reshape(16, 16, 16, 16).any(axis=(1, 3))
    assert tiles.sum() > 50                                                                # of the last view's 256 tiles


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
def test_new_abi_surface():
    from d3ga_amd import _lib
    src = open(os.path.join(ROOT, "include", "d3ga.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], capture_output=True, text=True, check=True).stdout
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert hasattr(_lib.lib(), name)
        assert re.search(r"\bT %s$" % name, out, flags=re.M), name
    assert sorted(n for n in _lib.EXPORTS if n.startswith("d3ga_points_")) == sorted(NEW_EXPORTS)
    assert sorted(set(re.findall(r"\b(d3ga_points_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))) == sorted(NEW_EXPORTS)
    assert "d3ga_*" in open(os.path.join(ROOT, "d3ga_amd", "csrc", "d3ga.map")).read()
    assert _lib.ABI_VERSION == 112 and re.search(r"#define\s+D3GA_VERSION\s+112\b", src) and _lib.lib().d3ga_version() == 112
    assert _lib.POINTS_MAX_K == 8 == int(re.search(r"#define\s+D3GA_POINTS_MAX_K\s+(\d+)", src).group(1))
    build = open(os.path.join(ROOT, "d3ga_amd", "csrc", "build.py")).read()
    assert "point_raster.hip" in build and "point_raster_math.h" in build
    from d3ga_amd.csrc import build as b
    assert b.EXTRA["point_raster.hip"] == b.EXTRA["mesh_raster.hip"] and "-ffp-contract=off" in b.EXTRA["point_raster.hip"]
    assert [len(_lib._SIGNATURES[k][0]) for k in NEW_EXPORTS] == [6, 13, 12]
    import d3ga_amd
    for name in ("PCRenderer", "PointScratch", "PointFragments", "rasterize_points"):
        assert hasattr(d3ga_amd, name) and name in d3ga_amd.__all__
    assert d3ga_amd.PCRenderer.to_cameras is d3ga_amd.to_cameras


def test_scratch_bytes():
    from d3ga_amd import _lib
    f = _lib.lib().d3ga_points_raster_scratch_bytes
    n = ctypes.c_size_t()
    assert f(1, 1, 8, 8, 0.007, ctypes.byref(n)) == 0 and n.value >= 16 + 2 * 4 * 256 + 4 + 16
    # 135 000 points at 747 x 1022, r_px = 2.61: at most 2 x 2 tiles per point
    assert f(1, 135000, 747, 1022, 0.007, ctypes.byref(n)) == 0 and 135000 * 4 * 16 <= n.value <= 135000 * 4 * 16 + 64 * 1024
    assert f(0, 0, 1, 1, 0.007, ctypes.byref(n)) == 0 and n.value >= 16
    assert f(1, 1000, 64, 64, 100.0, ctypes.byref(n)) == 0 and n.value <= 1000 * 16 * 16 + 64 * 1024       # never more than the frame's tiles
    assert f(1, 1, 16384, 16384, 0.007, ctypes.byref(n)) == 0 and n.value >= 2 * 4 * 1024 * 1024
    assert f(1, 1, 8, 8, 0.007, None) == E_NULL
    for kw in ((-1, 1, 8, 8), (1, -1, 8, 8), (1, 1, 0, 8), (1, 1, 8, 0), (1, 1, 16385, 8), (1, 1, 8, 16385), (2, 2 ** 30, 8, 8),
               (2 ** 16, 2 ** 15, 8, 8)):
        assert f(*kw, 0.007, ctypes.byref(n)) == E_SIZE, kw
    assert f(1, 2 ** 31 - 1, 8, 8, 0.007, ctypes.byref(n)) == 0
    assert f(1, 2 ** 30, 16384, 16384, 1.0, ctypes.byref(n)) == E_SIZE                                     # lists beyond 2^36 records
    for radius in (0.0, -0.007, float("nan"), float("inf")):
        assert f(1, 1, 8, 8, radius, ctypes.byref(n)) == E_CONFIG, radius


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """The refusals happen before any HIP call: host buffers stand in for device memory and are never touched."""
    from d3ga_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    odd = ctypes.c_void_p(p.value + 2)
    bg = (ctypes.c_float * 3)(1, 1, 1)
    sizes = dict(B=1, P=3, H=2, W=2, K=5, radius=0.007)
    bad_sizes = [dict(B=-1), dict(P=-1), dict(H=0), dict(W=0), dict(H=-4), dict(H=16385), dict(W=16385), dict(B=2, P=2 ** 30)]
    bad_settings = [dict(K=0), dict(K=9), dict(K=-1), dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf"))]
    calls = {
        "rasterize": (L.d3ga_points_rasterize, dict(**sizes, points=p, cams=p, scratch=p, idx=p, zbuf=p, dists=p),
                      ("points", "cams", "scratch", "idx"), ("zbuf", "dists")),
        "composite": (L.d3ga_points_composite, dict(**sizes, idx=p, dists=p, colors=p, bg=bg, image=p), ("idx", "dists", "bg", "image"), ("colors",)),
    }
    for what, (fn, ok, required, optional) in calls.items():
        call = lambda **kw: fn(*{**ok, **kw}.values(), None)
        for kw in bad_sizes:
            assert call(**kw) == E_SIZE, (what, kw)
        for kw in bad_settings:
            assert call(**kw) == E_CONFIG, (what, kw)
        for name in required:
            assert call(**{name: None}) == E_NULL, (what, name)
        for name in required + optional:
            if name != "bg":
                assert call(**{name: odd}) == E_CONFIG, (what, name)
        assert call(B=0) == 0                                                                    # nothing to do, nothing launched
    call = lambda **kw: L.d3ga_points_rasterize(*{**calls["rasterize"][1], **kw}.values(), None)
    assert call(scratch=ctypes.c_void_p(p.value + 8)) == E_CONFIG                                # 16-byte alignment
    assert call(B=0, P=0, points=None) == 0
    assert call(P=2 ** 30, H=16384, W=16384, radius=1.0) == E_SIZE
    assert not any(buf)


def test_python_layer_validates_on_the_host():
    from d3ga_amd import D3GAError, MeshCameras, PCRenderer, PointScratch, rasterize_points
    cams = MeshCameras(np.eye(3), np.zeros(3), np.diag([8.0, 8.0, 1.0]), (6, 8), device="cpu")
    two = MeshCameras(np.eye(3), np.zeros((2, 3)), np.eye(3), (6, 8), device="cpu")
    verts = torch.zeros(1, 4, 3)
    r = PCRenderer()
    assert (r.radius, r.points_per_pixel, r.white_background) == (0.007, 5, True) and list(r._bg) == [1.0, 1.0, 1.0]
    assert list(PCRenderer(white_background=False)._bg) == [0.0, 0.0, 0.0] and r.cuda() is r       # the reference's PCRenderer(...).cuda()
    assert float(np.abs(np.array(PCRenderer.DEFAULT_COLOR) - pr.DEFAULT_COLOR).max()) == 0
    sized = PCRenderer(white_background=False, radius=0.01, points_per_pixel=8)
    sized.resize(6, 9)
    bad = [
        lambda: PCRenderer(points_per_pixel=0),                                                 # settings
        lambda: PCRenderer(points_per_pixel=9),
        lambda: PCRenderer(points_per_pixel=2.5),
        lambda: PCRenderer(points_per_pixel=True),
        lambda: PCRenderer(radius=0),
        lambda: PCRenderer(radius=-0.007),
        lambda: PCRenderer(radius=float("nan")),
        lambda: PCRenderer(radius=float("inf")),
        lambda: PCRenderer(radius=1e-60),                                                       # 0 as a float32
        lambda: PCRenderer(radius="wide"),
        lambda: rasterize_points(cams, verts, radius=0.0),
        lambda: rasterize_points(cams, verts, points_per_pixel=9),
        lambda: PointScratch(1, 4, 6, 8, 0, 0.007, device="cpu"),
        lambda: r.render(None, verts),                                                          # cameras
        lambda: r.render(two, verts),
        lambda: r.render(cams, verts[0]),                                                       # vertices
        lambda: r.render(cams, verts.double()),
        lambda: r.render(cams, verts.numpy()),
        lambda: r.render(cams, torch.zeros(1, 4, 2)),
        lambda: r.rasterize_points(cams, verts[0]),
        lambda: sized(cams, verts),                                                             # resize disagrees with the cameras
        lambda: sized.render(cams, verts),
        lambda: sized.rasterize_points(cams, verts),
        lambda: sized.resize(0, 4),
        lambda: r.resize(4, 16385),
    ]
    for i, fn in enumerate(bad):
        with pytest.raises(ValueError):
            fn()
            pytest.fail(f"case {i} was accepted")
    # everything fits, but the tensors live on the CPU: require_cuda's refusal, a ValueError and a D3GAError at once
    for fn in (lambda: r(cams, verts), lambda: r.forward(cams, verts), lambda: r.render(cams, verts, torch.zeros(4, 3)),
               lambda: r.rasterize_points(cams, verts), lambda: rasterize_points(cams, verts)):
        with pytest.raises(ValueError) as info:
            fn()
        assert isinstance(info.value, D3GAError) and "GPU only" in str(info.value)
    from d3ga_amd.point_render import PointRenderDeviceError
    assert issubclass(PointRenderDeviceError, D3GAError) and issubclass(PointRenderDeviceError, ValueError)
