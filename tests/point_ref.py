"""Float64 numpy oracle of the point-cloud rasterizer and compositor (d3ga_amd/point_render.py, csrc/point_raster.hip),
written from the semantics section of DESIGN.md 4.4h, the inputs of its tests, and the g++ build of csrc/point_raster_math.h
(tests/hostcheck/pointcheck.cpp) both test modules run.

rasterize_ref is a brute force over every (pixel, point) pair.  Besides the fragments it flags the MARGINAL pixels no float32
implementation can be held to:
  * a pixel where some kept point has |dist2 / radius^2 - 1| < MEMBER_EDGE (the pixel centre sits on a disc's rim), and
  * a pixel where two adjacent depths among its K + 1 nearest members differ by less than DEPTH_GAP * z -- unless the two
    points have the very same float32 coordinates: then every implementation computes the same depth for both and the tie
    rule (the smaller index first) decides, which is held exactly.  (This asks more than flagging every small gap would.)
Both thresholds are about ten times the float32 error for frames up to 128 px on a side: a projection error of about 3e-5 px at
r_px = 2.6 moves dist2 / radius^2 by about 2e-5; a view depth near z = 3 is good to about 2e-7 relative.
Away from the marginal pixels idx must be exactly the oracle's.  On them every chosen point must have
dist2 / radius^2 < 1 + MEMBER_EDGE.
"""
import ctypes
import os
import subprocess

import numpy as np

from mesh_ref import cam_row, look_at

MEMBER_EDGE = 1e-4
DEPTH_GAP = 2e-6
MARGINAL_CAP = 0.03          # of the covered pixels, in every case
NEAR = 0.01
DEFAULT_COLOR = np.array([154.0, 205.0, 50.0]) / 255.0

# Value bars: 8 x the largest deviation of the g++ build of csrc/point_raster_math.h (-ffp-contract=off, tests/hostcheck/
# pointcheck.cpp) from this oracle on the non-marginal pixels of ALL cases below, rounded up to two digits
# (tests/test_point_render_host.py::test_host_build_equals_the_oracle prints the measured values and holds the host build to
# bar / 8).  zbuf relative to the depth, dists relative to radius^2 (so both are dimensionless), image in colour units.
# image was 1.3e-5 (the 0.6-pixel discs) until the 256-pixel frames came: tiles256 measures 1.64e-5 there (its dists 1.65e-5: u
# and v near 250 carry twice the rounding error they carry in a 90-pixel frame), tiles272 1.36e-5.  The other two are unchanged.
MEASURED = {"zbuf_rel": 9.2e-8, "dists": 1.8e-5, "image": 1.7e-5}
BARS = {k: 8 * v for k, v in MEASURED.items()}


# ---- scenes -------------------------------------------------------------------------------------------------------------
def shell(P, seed):
    """P points on a bumpy sphere of radius about 1 -> (P,3) float32"""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((P, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = 1 + 0.06 * np.cos(3 * d[:, 0] + 1) * np.cos(2 * d[:, 1] + 2) + 0.04 * np.sin(4 * d[:, 2]) + 0.01 * rng.uniform(-1, 1, P)
    return (d * r[:, None]).astype(np.float32)


def solid(P, seed):
    """P points uniformly inside an ellipsoid of half axes (1, 0.75, 0.55) -> (P,3) float32"""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((P, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (d * np.cbrt(rng.random(P))[:, None] * [1.0, 0.75, 0.55]).astype(np.float32)


def camera(H, W, dist=3.0, direction=(0.3, 0.4, -1.0), fill=0.45):
    """A camera at `dist` from the origin that shows the unit ball over `fill` of the shorter side."""
    d = np.asarray(direction, np.float64)
    R, t = look_at(dist * d / np.linalg.norm(d))
    f = fill * min(H, W) * np.sqrt(dist * dist - 1.21) / 1.1
    return cam_row(R, t, f, 1.03 * f, 0.5 * W + 0.3, 0.5 * H - 0.2)


def radius_of(r_px, H, W):
    """The NDC radius (a float32 value, as the entry points take it) of a disc of r_px pixels."""
    return float(np.float32(2.0 * r_px / min(H, W)))


def _one(points, cam, H, W, r_px, K=5):
    return dict(points=np.ascontiguousarray(points, np.float32)[None], cams=np.ascontiguousarray(cam, np.float32)[None], H=H, W=W,
                radius=radius_of(r_px, H, W), K=K)


def make_case(name):
    """-> dict(points (B,P,3) float32, cams (B,16) float32, H, W, radius, K)"""
    if name in ("shell_70x90", "shell_90x70", "solid_70x90", "solid_90x70"):
        H, W = (70, 90) if name.endswith("70x90") else (90, 70)
        pts = shell(3000, 31) if name.startswith("shell") else solid(3000, 32)
        return _one(pts, camera(H, W), H, W, 2.6)
    if name == "dense6000":                                   # the busiest tile list runs over three LDS batches of 256
        return _one(solid(6000, 33), camera(70, 90, direction=(1.0, 0.1, 0.2)), 70, 90, 2.6)
    if name == "wide_discs":                                  # a 3 x 3 tile grid, boxes of 9 pixels: up to 2 x 2 tiles each
        return _one(shell(500, 34), camera(33, 47, direction=(-0.5, 0.2, -1.0)), 33, 47, 4.0)
    if name == "wider_discs":                                 # boxes of 19 pixels: up to 3 x 3 tiles each
        return _one(shell(150, 44), camera(33, 47, direction=(-0.5, 0.2, -1.0)), 33, 47, 9.0)
    if name == "narrow_discs":                                # most discs miss every pixel centre
        return _one(shell(3000, 35), camera(70, 90), 70, 90, 0.6)
    if name == "duplicates":                                  # 200 of 300 points twice, with the very same coordinates
        base = shell(300, 36)
        pts = np.concatenate([base, base[:200]])[np.random.default_rng(37).permutation(500)]
        return _one(pts, camera(70, 90), 70, 90, 2.6)
    if name == "behind_and_outside":                          # a close-up: most of the shell outside the frame; points behind the camera
        cam = camera(70, 90, dist=2.2, fill=1.6)
        R, t = cam[:9].reshape(3, 3).astype(np.float64), cam[9:12].astype(np.float64)
        rng = np.random.default_rng(38)
        view = np.concatenate([rng.uniform(-1, 1, (300, 3)) * [0.5, 0.5, 1.0] - [0, 0, 1.2],        # z < 0
                               rng.uniform(-1, 1, (50, 3)) * [0.002, 0.002, 0.004] + [0, 0, 0.005]])  # 0 < z < 0.01: dropped too
        behind = (view - t) @ R
        return _one(np.concatenate([shell(1500, 39), behind.astype(np.float32)]), cam, 70, 90, 2.6)
    if name == "k1":
        return _one(shell(3000, 31), camera(70, 90), 70, 90, 2.6, K=1)
    if name == "k8":
        return _one(solid(3000, 32), camera(70, 90), 70, 90, 2.6, K=8)
    if name == "one_point":
        return _one(np.array([[0.1, -0.05, 0.2]], np.float32), camera(33, 47), 33, 47, 2.6)
    if name == "batch3":                                      # three clouds, three cameras
        pts = np.stack([shell(1000, 41), solid(1000, 42), shell(1000, 43)])
        cams = np.stack([camera(37, 53, 3.0, d) for d in ((0.3, 0.4, -1.0), (-1.0, 0.1, 0.3), (0.1, -0.8, 0.7))])
        return dict(points=pts, cams=cams, H=37, W=53, radius=radius_of(2.6, 37, 53), K=5)
    if name in ("k2", "k3", "k4", "k6", "k7"):                # every instantiation of the tile kernel: k8's cloud and camera
        return _one(solid(3000, 32), camera(70, 90), 70, 90, 2.6, K=int(name[1]))
    # The tile table is built in workgroups of 256 tiles (TABLE_BLOCK): a tile's list begins at block_start[t / 256] + local[t]
    # and ends where tile t + 1's begins, or at block_start[nblk] behind the very last padded slot.
    if name == "tiles256":                                    # 16 x 16 tiles: one full table workgroup, the last tile ends at block_start[nblk]
        return _one(shell(6000, 51), camera(256, 256), 256, 256, 2.6)
    if name == "tiles272":                                    # 17 x 16 tiles: two table workgroups, tile 255 ends where the second begins
        return _one(shell(6000, 52), camera(272, 256), 272, 256, 2.6)
    if name == "views3_330":                                  # 3 views of 10 x 11 tiles: the table boundary (tile 256) inside view 2,
        pts = np.stack([shell(3000, 61), solid(3000, 62), shell(3000, 63)])                    # the view boundaries inside workgroup 0
        cams = np.stack([camera(160, 176, 3.0, d) for d in ((0.3, 0.4, -1.0), (-1.0, 0.1, 0.3), (0.1, -0.8, 0.7))])
        return dict(points=pts, cams=cams, H=160, W=176, radius=radius_of(2.6, 160, 176), K=5)
    if name == "views257":                                    # 257 views of one tile each: the second table workgroup holds one tile
        dirs = np.random.default_rng(99).standard_normal((257, 3))
        pts = np.stack([shell(40, 100 + b) for b in range(257)])
        cams = np.stack([camera(16, 16, 3.0, d) for d in dirs])
        return dict(points=pts, cams=cams, H=16, W=16, radius=radius_of(1.5, 16, 16), K=5)
    # Not in CASES (no full oracle: tests/test_gpu_point_render.py::test_a_quarter_million_one_pixel_views samples them).
    if name == "pixels262400":                                # 262 400 views of one pixel: 1025 table workgroups (the scan kernel's second
        B, P = PIXEL_VIEWS, 4                                 # trip, with a carry), four to five grid-stride trips of the tile kernel
        rng = np.random.default_rng(71)
        pts = (PIXEL_SPREAD * rng.standard_normal((B, P, 3))).astype(np.float32)
        cams = np.repeat(camera(1, 1, fill=0.6)[None], B, 0)
        cams[:, 14] += rng.uniform(-0.3, 0.3, B).astype(np.float32)
        return dict(points=pts, cams=cams, H=1, W=1, radius=radius_of(0.6, 1, 1), K=5)
    if name == "views257_k1":                                 # 257 x 256 = 65 792 tiles: 256 tile workgroups make a second trip
        rng = np.random.default_rng(72)
        dirs = rng.standard_normal((257, 3))
        d = rng.standard_normal((257, 200, 3))
        pts = (d / np.linalg.norm(d, axis=2, keepdims=True)).astype(np.float32)
        cams = np.stack([camera(256, 256, 3.0, d) for d in dirs])
        return dict(points=pts, cams=cams, H=256, W=256, radius=radius_of(2.6, 256, 256), K=1)
    raise KeyError(name)


TABLE_BLOCK = 256            # tiles per workgroup of the tile table (kBlock of csrc/point_raster.hip)
PIXEL_VIEWS = 1025 * 256     # more table workgroups than one trip of the scan kernel (1024), more tiles than tile workgroups (65 536)
# sigma of the one-pixel views' clouds: between a quarter and three quarters of the views have their pixel covered
# (tests/test_point_render_host.py::test_the_one_pixel_views_are_half_covered measures it with the host build)
PIXEL_SPREAD = 2.0

CASES = ("shell_70x90", "shell_90x70", "solid_70x90", "solid_90x70", "dense6000", "wide_discs", "wider_discs", "narrow_discs", "duplicates",
         "behind_and_outside", "k1", "k8", "one_point", "batch3", "tiles256", "tiles272", "views3_330", "views257", "k2", "k3", "k4", "k6",
         "k7")


def n_tiles(case):
    """tiles of a case, all views"""
    return len(case["points"]) * ((case["H"] + 15) // 16) * ((case["W"] + 15) // 16)


def point_colours(case, seed=3):
    B, P = case["points"].shape[:2]
    return np.random.default_rng(seed).random((B, P, 3)).astype(np.float32)


# ---- the oracle ---------------------------------------------------------------------------------------------------------
def project_ref(points, cam):
    """float64 (u, v, z, keep) of a cloud as stored (float32)"""
    p = np.asarray(points, np.float64)
    cam = np.asarray(cam, np.float64)
    R, t, (fx, fy, cx, cy) = cam[:9].reshape(3, 3), cam[9:12], cam[12:16]
    vc = p @ R.T + t
    z = vc[:, 2]
    keep = z > NEAR
    zs = np.where(keep, z, 1.0)
    return fx * vc[:, 0] / zs + cx, fy * vc[:, 1] / zs + cy, z, keep


def rasterize_ref(points, cam, H, W, radius, K):
    """One cloud, one camera row; inputs as stored (float32), arithmetic in float64, every (pixel, point) pair visited.
    -> dict: idx (H,W,K) int64, zbuf, dists (H,W,K) with -1 in the empty slots, marginal (H,W) bool, covered (H,W) bool
    (slot 0 filled), members (H,W): points per pixel."""
    u, v, z, keep = project_ref(points, cam)
    P = len(z)
    s2, r2 = (2.0 / min(H, W)) ** 2, float(radius) ** 2
    marginal = np.zeros((H, W), bool)
    pix_l, pt_l, d_l = [], [], []
    cols = np.arange(W) + 0.5
    for j in range(H):
        d2 = ((cols[:, None] - u[None, :]) ** 2 + ((j + 0.5 - v) ** 2)[None, :]) * s2          # (W,P)
        ratio = d2 / r2
        marginal[j] = ((np.abs(ratio - 1) < MEMBER_EDGE) & keep[None, :]).any(1)
        ii, pp = np.nonzero((ratio < 1) & keep[None, :])
        pix_l.append(j * W + ii); pt_l.append(pp); d_l.append(d2[ii, pp])
    pix, pt, d2 = np.concatenate(pix_l), np.concatenate(pt_l), np.concatenate(d_l)
    idx = np.full((H * W, K), -1, np.int64)
    zbuf = np.full((H * W, K), -1.0)
    dists = np.full((H * W, K), -1.0)
    members = np.bincount(pix, minlength=H * W).reshape(H, W)
    if len(pix):
        order = np.lexsort((pt, z[pt], pix))                  # by pixel, then depth, then index
        pix, pt, d2 = pix[order], pt[order], d2[order]
        first = np.ones(len(pix), bool)
        first[1:] = pix[1:] != pix[:-1]
        start = np.maximum.accumulate(np.where(first, np.arange(len(pix)), 0))
        rank = np.arange(len(pix)) - start
        sel = rank < K
        idx[pix[sel], rank[sel]] = pt[sel]
        zbuf[pix[sel], rank[sel]] = z[pt[sel]]
        dists[pix[sel], rank[sel]] = d2[sel]
        # adjacent depths among the K + 1 nearest: entries of rank 1 .. K against their predecessors
        nxt = np.flatnonzero((rank >= 1) & (rank <= K))
        a, b = pt[nxt - 1], pt[nxt]
        close = (z[b] - z[a]) < DEPTH_GAP * z[a]
        pts32 = np.asarray(points, np.float32)
        same = (pts32[a] == pts32[b]).all(1)
        marginal.reshape(-1)[pix[nxt[close & ~same]]] = True
    return dict(idx=idx.reshape(H, W, K), zbuf=zbuf.reshape(H, W, K), dists=dists.reshape(H, W, K), marginal=marginal,
                covered=idx.reshape(H, W, K)[..., 0] >= 0, members=members)


def composite_ref(idx, dists, radius, colors=None, white=True):
    """AlphaCompositor over (H,W,K) fragments (float64) -> (H,W,3): sum_k w_k f_k prod_{j<k} (1 - w_j), the background only
    where slot 0 is empty."""
    H, W, K = idx.shape
    r2 = float(radius) ** 2
    img = np.zeros((H, W, 3))
    T = np.ones((H, W))
    for k in range(K):
        filled = idx[..., k] >= 0
        w = np.where(filled, 1.0 - dists[..., k] / r2, 0.0)
        f = DEFAULT_COLOR[None, None, :] if colors is None else np.asarray(colors, np.float64)[np.maximum(idx[..., k], 0)]
        img += (w * T)[..., None] * f
        T = T * (1.0 - w)
    img[idx[..., 0] < 0] = 1.0 if white else 0.0
    return img


class Reference:
    """The oracle's results of one case, element by element, and the checks the host build and the device share."""

    def __init__(self, name, case=None):
        self.name = name
        self.case = c = make_case(name) if case is None else case
        self.B, self.P = c["points"].shape[:2]
        self.H, self.W, self.K, self.radius = c["H"], c["W"], c["K"], c["radius"]
        self.colours = point_colours(c)
        self.frag = [rasterize_ref(c["points"][b], c["cams"][b], self.H, self.W, self.radius, self.K) for b in range(self.B)]

    def marginal_share(self):
        covered = sum(int(f["covered"].sum()) for f in self.frag)
        return sum(int((f["marginal"] & f["covered"]).sum()) for f in self.frag) / max(covered, 1), covered

    def check_fragments(self, idx, zbuf, dists):
        """(B,H,W,K) each -> {"zbuf_rel", "dists"}: the largest deviations on non-marginal pixels; idx is asserted: exact away
        from the marginal pixels, and on them no chosen point farther than the rim by more than MEMBER_EDGE."""
        dev = {"zbuf_rel": 0.0, "dists": 0.0}
        r2, s2 = float(self.radius) ** 2, (2.0 / min(self.H, self.W)) ** 2
        for b, ref in enumerate(self.frag):
            got = np.asarray(idx[b], np.int64)
            gz, gd = np.asarray(zbuf[b], np.float64), np.asarray(dists[b], np.float64)
            assert got.shape == ref["idx"].shape and ((got >= -1) & (got < self.P)).all()
            assert (gz[got < 0] == -1).all() and (gd[got < 0] == -1).all()
            m = ~ref["marginal"]
            bad = (got != ref["idx"]).any(-1) & m
            assert not bad.any(), f"{self.name}[{b}]: {int(bad.sum())} non-marginal pixels with other points, first at {np.argwhere(bad)[0]}"
            jj, ii, kk = np.nonzero((got >= 0) & ref["marginal"][..., None])
            if len(jj):
                u, v, z, keep = project_ref(self.case["points"][b], self.case["cams"][b])
                p = got[jj, ii, kk]
                ratio = ((ii + 0.5 - u[p]) ** 2 + (jj + 0.5 - v[p]) ** 2) * s2 / r2
                assert keep[p].all() and (ratio < 1 + MEMBER_EDGE).all(), f"{self.name}[{b}]: a marginal pixel holds a point beyond the rim"
            f = (ref["idx"] >= 0) & m[..., None]
            if f.any():
                dev["zbuf_rel"] = max(dev["zbuf_rel"], float((np.abs(gz[f] - ref["zbuf"][f]) / ref["zbuf"][f]).max()))
                dev["dists"] = max(dev["dists"], float(np.abs(gd[f] - ref["dists"][f]).max()) / r2)
        return dev

    def check_image(self, image, white, coloured):
        """(B,H,W,3) against the compositor at the oracle's fragments -> the largest deviation on non-marginal pixels; the
        background must be exact."""
        dev = 0.0
        for b, ref in enumerate(self.frag):
            want = composite_ref(ref["idx"], ref["dists"], self.radius, self.colours[b] if coloured else None, white)
            m = ~ref["marginal"]
            got = np.asarray(image[b], np.float64)
            assert (got[m & ~ref["covered"]] == (1.0 if white else 0.0)).all()
            dev = max(dev, float(np.abs(got[m] - want[m]).max()))
        return dev


_REFS = {}


def reference(name):
    """The oracle of a case, computed once per process."""
    if name not in _REFS:
        _REFS[name] = Reference(name)
    return _REFS[name]


def sampled_reference(name, every):
    """-> (views, the oracle of every `every`-th view of a case too large for a full one), computed once per process."""
    key = (name, every)
    if key not in _REFS:
        c = make_case(name)
        views = np.arange(0, len(c["points"]), every)
        _REFS[key] = (views, Reference(f"{name}[::{every}]", dict(c, points=c["points"][views], cams=c["cams"][views])))
    return _REFS[key]


_CASES = {}


def big_case(name, values=True):
    """make_case of one of the cases outside CASES with the host build's fragments (idx, zbuf, dists), once per process."""
    if name not in _CASES:
        c = make_case(name)
        _CASES[name] = (c,) + host_fragments(c, values=values)[:3]
    return _CASES[name]


# ---- the host build -----------------------------------------------------------------------------------------------------
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
_HOST = []


def host_lib():
    """tests/hostcheck/pointcheck.cpp as a shared library (g++ -ffp-contract=off, as meshcheck is built), once per process."""
    if not _HOST:
        src = os.path.join(ROOT, "tests", "hostcheck", "pointcheck.cpp")
        out_dir = os.path.join(ROOT, "tests", "hostcheck", "_build")
        os.makedirs(out_dir, exist_ok=True)
        so = os.path.join(out_dir, "libpointcheck.so")
        deps = [src, os.path.join(ROOT, "include", "d3ga.h")] + [os.path.join(ROOT, "d3ga_amd", "csrc", h) for h in ("point_raster_math.h", "mesh_raster_math.h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", so])
        lib = ctypes.CDLL(so)
        for fn in (lib.hc_points_rasterize, lib.hc_points_members_plain, lib.hc_points_members_tiled):
            fn.restype = ctypes.c_int64
        _HOST.append(lib)
    return _HOST[0]


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_fragments(case, reversed_lists=False, values=True):
    """The host build's fragments of a case -> (idx, zbuf, dists, the longest tile list); values=False: idx alone, zbuf and
    dists are None"""
    lib = host_lib()
    B, P = case["points"].shape[:2]
    H, W, K = case["H"], case["W"], case["K"]
    pts, cams = np.ascontiguousarray(case["points"]), np.ascontiguousarray(case["cams"])
    idx = np.full((B, H, W, K), -7, np.int32)
    zbuf, dists = (np.full((B, H, W, K), np.nan, np.float32), np.full((B, H, W, K), np.nan, np.float32)) if values else (None, None)
    longest = lib.hc_points_rasterize(B, P, H, W, K, ctypes.c_float(case["radius"]), _ptr(pts), _ptr(cams), int(reversed_lists), _ptr(idx),
                                      _ptr(zbuf), _ptr(dists))
    assert longest >= 0, longest
    return idx, zbuf, dists, int(longest)


def host_image(case, idx, dists, colours, white):
    lib = host_lib()
    B, P = case["points"].shape[:2]
    H, W, K = case["H"], case["W"], case["K"]
    bg = np.full(3, 1.0 if white else 0.0, np.float32)
    image = np.full((B, H, W, 3), np.nan, np.float32)
    lib.hc_points_composite(B, P, H, W, K, ctypes.c_float(case["radius"]), _ptr(idx), _ptr(dists), _ptr(colours), _ptr(bg), _ptr(image))
    return image
