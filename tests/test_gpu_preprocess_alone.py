"""The per-Gaussian kernels of d3ga_amd/csrc/raster_pre.hip on the device, alone: d3ga_raster_preprocess, then
d3ga_raster_preprocess_bwd on an accumulator the TEST fills -- no compositing launch -- through d3ga_amd._lib.lib() with raw
pointers, against float64 autograd of oracle/raster_torch.preprocess on the edge scenes of tests/preprocess_ref.py (which holds
the scenes, the reference and the bars; tests/test_preprocess_alone_host.py runs the same protocol on the g++ build).
  forward    radii = ceil(3 sqrt(lambda_max)) of the float64 reference on every row, 0 on culled rows; d3ga_selftest_alpha at the
             centre pixel and its four neighbours at +-2 of every visible Gaussian against the float64 opacity x aa x exp(-q / 2),
             where that lies in [2/255, 0.98] (no threshold decision enters): pins xy, conic and the stored opacity through `geom`.
  backward   every output of every row of ROWS and VIEW_ROWS under 4 e32 per Gaussian row (preprocess_ref.bars), culled rows,
             clamped channels, coefficients above the active degree and dL_dmeans2D[:, 2] exactly zero, dL_dmeans2D[:, :2] and --
             without antialiasing, identity activation -- dL_dopacity the accumulator's slots bit for bit.  The factored SH output
             goes through d3ga_sh_grad_from_views (one view) and must give the full block under the same bar.
  layout     the same Gaussians one per wavefront and behind 37 culled rows: gradient rows bit for bit the compact layout's.
geom / binning are sized by d3ga_raster_scratch_bytes_views / _window; radii, acc and every gradient sit between guard bands
(cage_ref.GuardedBuffer), checked after every call.  The measured ratios: docs/LOG.md, "Per-Gaussian kernels alone against float64"."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cage_ref as cr
import preprocess_ref as pr
from d3ga_amd import _lib
from d3ga_amd._lib import RasterParams

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OK = 0
WINDOW = (96, 80, 32, 32)               # w, h, ox, oy: the 64 x 48 window at the far corner of a 96 x 80 raster

# Pairwise cover of (colour path) x (covariance path) and (colour path) x (P); every value of every other axis at least once.
# id, P, M, degree (M = 0: precomputed colours), covariance, antialiasing, acc[:, 10] != 0, sigmoid activation, outputs, camera
#   outputs   full: dL_dsh | dL_dcolors;  factored: dL_dsh NULL, dL_dcolors given, then d3ga_sh_grad_from_views;
#             null: the full block, dL_dmeans2D and dL_dopacity NULL
#   camera    prm: tangents in the params;  slot: tanfovx = 0, tangents behind the position;  window: windowed slot (WINDOW)
ROWS = [
    ( 0,   1, 16, 0, "cov6", 0, 0, 0, "full", "prm"),
    ( 1,  65, 16, 0, "sr1", 0, 1, 1, "null", "slot"),
    ( 2, 209, 16, 0, "sr13", 1, 0, 0, "factored", "window"),
    ( 3, 257, 16, 0, "cov6", 1, 1, 1, "full", "prm"),
    ( 4,   1, 16, 1, "sr1", 1, 0, 1, "factored", "window"),
    ( 5,  65, 16, 1, "sr13", 1, 1, 0, "full", "prm"),
    ( 6, 209, 16, 1, "cov6", 0, 0, 1, "null", "slot"),
    ( 7, 257, 16, 1, "sr1", 0, 1, 0, "factored", "window"),
    ( 8,   1, 16, 2, "sr13", 0, 1, 0, "null", "slot"),
    ( 9,  65, 16, 2, "cov6", 0, 0, 1, "factored", "window"),
    (10, 209, 16, 2, "sr1", 1, 1, 0, "full", "prm"),
    (11, 257, 16, 2, "sr13", 1, 0, 1, "null", "slot"),
    (12,   1, 16, 3, "cov6", 1, 1, 1, "full", "slot"),
    (13,  65, 16, 3, "sr1", 1, 0, 0, "null", "window"),
    (14, 209, 16, 3, "sr13", 0, 1, 1, "factored", "prm"),
    (15, 257, 16, 3, "cov6", 0, 0, 0, "full", "slot"),
    (16,   1,  4, 1, "sr1", 0, 0, 1, "factored", "prm"),
    (17,  65,  4, 1, "sr13", 0, 1, 0, "full", "slot"),
    (18, 209,  4, 1, "cov6", 1, 0, 1, "null", "window"),
    (19, 257,  4, 1, "sr1", 1, 1, 0, "factored", "prm"),
    (20,   1,  9, 2, "sr13", 1, 0, 0, "null", "window"),
    (21,  65,  9, 2, "cov6", 1, 1, 1, "factored", "prm"),
    (22, 209,  9, 2, "sr1", 0, 0, 0, "full", "slot"),
    (23, 257,  9, 2, "sr13", 0, 1, 1, "null", "window"),
    (24,   1,  1, 0, "cov6", 0, 1, 1, "full", "window"),
    (25,  65,  1, 0, "sr1", 0, 0, 0, "null", "prm"),
    (26, 209,  1, 0, "sr13", 1, 1, 1, "factored", "slot"),
    (27, 257,  1, 0, "cov6", 1, 0, 0, "full", "window"),
    (28,   1,  0, 0, "sr1", 1, 1, 0, "full", "slot"),
    (29,  65,  0, 0, "sr13", 1, 0, 1, "null", "window"),
    (30, 209,  0, 0, "cov6", 0, 1, 0, "full", "prm"),
    (31, 257,  0, 0, "sr1", 0, 0, 1, "null", "slot"),
]
# Batches of views of shared geometry, a camera per view (preprocess_bwd_views_kernel; 9 views: a second group with `accum`; M = 9
# is not staged: per-view launches and d3ga_sh_grad_from_views inside the entry point).  frames: per_view_geometry.
# id, P, M, degree, covariance, antialiasing, sigmoid, n_views, frames
VIEW_ROWS = [
    ("v0", 209, 16, 3, "cov6", 0, 0, 2, 0),
    ("v1", 257, 16, 2, "sr13", 1, 1, 9, 0),
    ("v2", 65, 0, 0, "sr1", 0, 0, 9, 0),
    ("v3", 209, 9, 2, "cov6", 0, 1, 2, 0),
    ("v4", 65, 0, 0, "cov6", 1, 0, 2, 1),
]


def row_id(r):
    return "-".join(str(x) for x in r)


def L():
    return _lib.lib()


def S():
    return _lib.stream_handle()


def vp(x):
    if x is None:
        return None
    return ctypes.c_void_p(x.ptr() if isinstance(x, cr.GuardedBuffer) else x.data_ptr())


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype).contiguous()


def cfg_of(M, deg, cov, aa, sigmoid, camera="prm"):
    return pr.Cfg(M=M, deg=deg, from_sr=cov != "cov6", mod=1.3 if cov == "sr13" else 1.0, aa=bool(aa), sigmoid=bool(sigmoid),
                  window=WINDOW if camera == "window" else None)


@functools.lru_cache(maxsize=None)
def scene(P, seed, M, deg, cov, aa, sigmoid, camera, n_views):
    sc = pr.edge_scene(P, seed, cfg_of(M, deg, cov, aa, sigmoid, camera), n_views)
    pr.assert_classes(sc)
    return sc


class Run:
    """One d3ga_raster_preprocess + d3ga_raster_preprocess_bwd of `sc` on the device with guarded outputs."""

    def __init__(self, sc, acc, outputs="full", camera="prm", frames=False, arrays=None):
        cfg, k = sc["cfg"], len(sc["cams"])
        a = arrays or sc                                          # (the layout test hands rearranged rows)
        self.P = P = a["means3D"].shape[0]
        self.cfg, self.k = cfg, k
        tan = {"prm": (cfg.tanx, cfg.tany), "slot": (0.0, 0.0), "window": (-1.0, -1.0)}[camera]
        self.prm = prm = RasterParams(P=P, M=cfg.M, sh_degree=cfg.deg, W=cfg.W, H=cfg.H, tanfovx=tan[0], tanfovy=tan[1],
                                      scale_modifier=cfg.mod, antialiasing=int(cfg.aa), opacity_activation=int(cfg.sigmoid),
                                      n_views=k if k > 1 else 0, per_view_geometry=int(frames))
        cams = [pr.cam_arrays(c) for c in sc["cams"]]
        tail = {"prm": [], "slot": [cfg.tanx, cfg.tany], "window": [cfg.tanx, cfg.tany, *map(float, WINDOW)]}[camera]
        self.view, self.proj = dev(np.stack([c[0] for c in cams])), dev(np.stack([c[1] for c in cams]))
        self.campos = dev(np.stack([np.concatenate([c[2], np.asarray(tail, np.float32)]) for c in cams]))
        rep = (lambda x: np.stack([x] * k)) if frames else (lambda x: x)       # a batch of frames: every view its own (equal) geometry
        self.means = dev(rep(a["means3D"]))
        self.shs = dev(a["shs"][:, :cfg.M]) if cfg.sh else None
        self.colors = None if cfg.sh else dev(a["rgb"])
        self.opac = dev(a["logits"] if cfg.sigmoid else a["opacities"])
        self.scales, self.rots = (dev(rep(a["scales"])), dev(rep(a["rotations"]))) if cfg.from_sr else (None, None)
        self.cov6 = None if cfg.from_sr else dev(rep(a["cov6"]))
        cap, sizes = 16384 * k, (ctypes.c_int64 * 3)()
        fn = L().d3ga_raster_scratch_bytes_window if camera == "window" else L().d3ga_raster_scratch_bytes_views
        assert fn(P, cfg.W, cfg.H, k, cap, 0, sizes) == OK
        self.geom = torch.zeros(int(sizes[0]), dtype=torch.uint8, device=DEV)
        self.binning = torch.zeros(int(sizes[1]), dtype=torch.uint8, device=DEV)
        self.radii = cr.GuardedWords("radii", (k * P,), DEV)
        p = ctypes.byref(prm)
        st = L().d3ga_raster_preprocess(p, vp(self.means), vp(self.shs), vp(self.colors), vp(self.opac), vp(self.scales), vp(self.rots),
                                        vp(self.cov6), vp(self.view), vp(self.proj), vp(self.campos), vp(self.geom), vp(self.binning), cap,
                                        vp(self.radii), S())
        assert st == OK, st
        torch.cuda.synchronize()
        self.radii.check()
        assert int(self.binning[:8].view(torch.int32)[1]) == 0, "tile lists truncated"
        if acc is None:
            return
        self.acc = cr.GuardedBuffer("acc", (k * P, pr.ACC_STRIDE), DEV)
        self.acc.t.copy_(dev(acc))
        kg = k if frames else 1
        G = lambda name, *shape: cr.GuardedBuffer(name, shape, DEV)
        sh_full = cfg.sh and outputs != "factored"
        self.g = g = dict(means3D=G("dL_dmeans3D", kg * P, 3), m2=None if outputs == "null" else G("dL_dmeans2D", k * P, 3),
                          opacities=None if outputs == "null" else G("dL_dopacity", P, 1),
                          sh=G("dL_dsh", P, cfg.M, 3) if sh_full else None,
                          colors=G("dL_dcolors", P, 3) if (not cfg.sh or outputs == "factored") else None,
                          cov3D=None if cfg.from_sr else G("dL_dcov3D", kg * P, 6),
                          scales=G("dL_dscales", kg * P, 3) if cfg.from_sr else None, rotations=G("dL_drots", kg * P, 4) if cfg.from_sr else None)
        # a batch of views with SH colours: the (k, P, 3) per-view factors the entry point may use on its way to dL_dsh (scratch)
        factors = torch.zeros(k * P, 3, device=DEV) if (cfg.sh and k > 1) else g["colors"]
        st = L().d3ga_raster_preprocess_bwd(p, vp(self.means), vp(self.shs), vp(self.scales), vp(self.rots), vp(self.cov6), vp(self.view),
                                            vp(self.proj), vp(self.campos), vp(self.geom), vp(self.acc), vp(g["means3D"]), vp(g["m2"]),
                                            vp(g["opacities"]), vp(g["sh"]), vp(factors), vp(g["cov3D"]), vp(g["scales"]),
                                            vp(g["rotations"]), S())
        assert st == OK, st
        torch.cuda.synchronize()
        for b in g.values():
            if b is not None:
                b.check()
        self.acc.check()
        assert torch.equal(self.acc.t.cpu(), torch.from_numpy(acc)), "the accumulator was written (acc_self_clearing = 0)"
        if cfg.sh and outputs == "factored" and k == 1:           # the full block from the (P, 3) factor, one view
            self.factor = g["colors"]
            g["sh"] = G("dL_dsh", P, cfg.M, 3)
            st = L().d3ga_sh_grad_from_views(P, cfg.M, cfg.deg, 1, vp(self.means), vp(self.factor), 3 * P, vp(self.campos),
                                             self.campos.shape[1], 1.0, vp(g["sh"]), S())
            assert st == OK, st
            torch.cuda.synchronize()
            g["sh"].check()
            self.factor.check()
            g["colors"] = None                                    # (an SH row has no `colors` reference: the factor is judged through the block)

    def got(self):
        return {key: None if b is None else b.t.cpu().numpy() for key, b in self.g.items()}


def check_alpha(run, sc, f64, f32):
    """d3ga_selftest_alpha on the records `run` left, at five pixels per visible Gaussian, against the float64 alpha."""
    cfg, vis = sc["cfg"], f64["vis"]
    rows = np.nonzero(vis)[0]
    if not len(rows):
        return
    off = np.array([[0, 0], [2, 0], [-2, 0], [0, 2], [0, -2]])
    gid = np.repeat(rows, 5)
    pix = np.rint(f64["xy"][gid]).astype(np.int64) + np.tile(off, (len(rows), 1))

    def alpha(f):
        d = f["xy"][gid].astype(np.float64) - pix
        cn = f["conic"][gid].astype(np.float64)
        return f["opacity"][gid].astype(np.float64) * np.exp(-0.5 * (cn[:, 0] * d[:, 0] ** 2 + cn[:, 2] * d[:, 1] ** 2) - cn[:, 1] * d[:, 0] * d[:, 1])
    a64, a32 = alpha(f64), alpha(f32)
    keep = (a64 >= 2.0 / 255.0) & (a64 <= 0.98) & (pix[:, 0] >= 0) & (pix[:, 0] < cfg.W) & (pix[:, 1] >= 0) & (pix[:, 1] < cfg.H)
    gid, pix, a64, a32 = gid[keep], pix[keep], a64[keep], a32[keep]
    n = len(gid)
    if n == 0:
        return
    ok, al = torch.zeros(n, dtype=torch.uint8, device=DEV), torch.full((n,), float("nan"), device=DEV)
    d_gid, d_px, d_py = dev(gid, torch.int32), dev(pix[:, 0], torch.int32), dev(pix[:, 1], torch.int32)      # (kept alive over the launch)
    st = L().d3ga_selftest_alpha(run.P, vp(run.geom), n, vp(d_gid), vp(d_px), vp(d_py), vp(ok), vp(al), S())
    assert st == OK, st
    torch.cuda.synchronize()
    grp = pr.groups(sc)[gid]
    rel32 = np.abs(a32 - a64) / a64
    e_all = max(pr.E32_FLOOR, float(rel32.max()))
    e = np.array([max(pr.E32_FLOOR, float(rel32[grp == c].max())) if (grp == c).sum() >= pr.MIN_GROUP else e_all for c in grp])
    ratio = np.abs(al.cpu().numpy().astype(np.float64) - a64) / (e * a64)
    i = int(np.argmax(ratio))
    print(f"[preprocess-alone] alpha at {n} pixels of {len(rows)} Gaussians: worst x{ratio[i]:.2f} of its class's e32 = {e[i]:.2e} "
          f"({sc['kind'][gid[i]]}), the scene's e32 {e_all:.2e}")
    assert bool(ok.all()), "a pixel with alpha in [2/255, 0.98] is not touched"
    assert ratio[i] <= pr.MARGIN, (ratio[i], e[i], sc["kind"][gid[i]])


@pytest.mark.parametrize("row", ROWS, ids=[row_id(r) for r in ROWS])
def test_single_view_row(row):
    n, P, M, deg, cov, aa, invd, sigmoid, outputs, camera = row
    sc = scene(P, 500 + n, M, deg, cov, aa, sigmoid, camera, 1)
    cfg = sc["cfg"]
    acc = pr.make_acc(P, 900 + n, bool(invd))
    ref64, refs32 = pr.reference(sc, cfg, acc, torch.float64), pr.references32(sc, cfg, acc)
    e32 = pr.bars(ref64, refs32, sc)
    run = Run(sc, acc, outputs, camera)
    # forward
    np.testing.assert_array_equal(run.radii.t.cpu().numpy(), ref64["radii_full"])
    if camera != "window":                                        # (a windowed record's pixel coordinates are the full raster's)
        check_alpha(run, sc, pr.forward64(sc, cfg, sc["cams"][0]), pr.forward64(sc, cfg, sc["cams"][0], dtype=torch.float32))
    # backward
    got = run.got()
    pr.check_grads(got, ref64, e32, sc, cfg, acc, f"device row {row_id(row)}", m2=got["m2"])
    if outputs == "factored" and cfg.sh:                          # the factor itself: the clamp-masked dL/dcolour, exactly
        vis, f = ref64["vis"], run.factor.t.cpu().numpy()
        want = np.where(ref64["clamped"] | ~vis[:, None], np.float32(0), acc[:, 7:10])
        np.testing.assert_array_equal(f, want)


@pytest.mark.parametrize("row", VIEW_ROWS, ids=[row_id(r) for r in VIEW_ROWS])
def test_views_row(row):
    """The float64 sum over the views' references (per view for what a batch of frames writes per view); culling differs between
    the views."""
    name, P, M, deg, cov, aa, sigmoid, k, frames = row
    sc = scene(P, 700 + VIEW_ROWS.index(row), M, deg, cov, aa, sigmoid, "prm", k)
    cfg = sc["cfg"]
    acc = pr.make_acc(P, 950 + VIEW_ROWS.index(row), True, views=k)
    accs = [acc[v * P:(v + 1) * P] for v in range(k)]
    r64 = [pr.reference(sc, cfg, accs[v], torch.float64, view=v) for v in range(k)]
    r32 = [pr.references32(sc, cfg, accs[v], view=v) for v in range(k)]
    visv = np.stack([r["vis"] for r in r64])
    assert (visv.any(0) & ~visv.all(0)).sum() >= 4, "culling does not differ between the views"
    run = Run(sc, acc, "full", "prm", frames=bool(frames))
    np.testing.assert_array_equal(run.radii.t.cpu().numpy().reshape(k, P), np.stack([r["radii"] for r in r64]))
    got = run.got()
    m2 = got.pop("m2").reshape(k, P, 3)
    for v in range(k):
        vis = r64[v]["vis"]
        assert np.array_equal(m2[v][vis, :2], accs[v][vis, :2]) and np.all(m2[v][~vis] == 0) and np.all(m2[v][:, 2] == 0), f"dL_dmeans2D of view {v}"
    geo = ("means3D", "cov3D", "scales", "rotations")
    if frames:                                                    # geometry gradients per view, appearance summed
        for v in range(k):
            pr.check_grads({key: got[key].reshape(k, P, -1)[v] for key in geo if got.get(key) is not None}, r64[v], pr.bars(r64[v], r32[v], sc),
                           sc, cfg, accs[v], f"device views {name} frame {v}", opacity_exact=False)
        got = {key: val for key, val in got.items() if key not in geo}
    s64 = pr.sum_views(r64)
    s32 = [pr.sum_views([r32[v][j] for v in range(k)]) for j in range(len(r32[0]))]
    if frames:
        for key in geo:
            s64.pop(key, None)
    pr.check_grads(got, s64, pr.bars(s64, s32, sc), sc, cfg, acc, f"device views {name} ({k} views)", opacity_exact=False)


def test_gradient_rows_do_not_depend_on_the_layout():
    """64 Gaussians as one full wavefront (the full48 slab), then behind 37 culled rows (a full wavefront and a partial one), then
    four of them one per wavefront among culled rows: every gradient row bit for bit the compact layout's.  Staged SH (M = 16).
    The regression test of sh_accumulate_jacobian's rounding: while the compiler was free to contract it, dL/dmeans3D of 6 of the 37
    Gaussians that moved into the partial wavefront differed from the compact layout's by up to 6.8e-8 of the row's largest element
    (the forward's full-wavefront path and its slab path had left different last bits in d(colour)/d(direction))."""
    sc = scene(64, 640, 16, 3, "cov6", 1, 0, "prm", 1)
    cfg = sc["cfg"]
    acc = pr.make_acc(64, 641, True)
    keys = ("means3D", "shs", "rgb", "opacities", "logits", "scales", "rotations", "cov6")
    behind = int(np.nonzero(sc["kind"] == "behind")[0][0])
    base = Run(sc, acc).got()
    assert pr.reference(sc, cfg, acc, torch.float64)["vis"].sum() >= 48

    def place(rows_at, P):
        arrays = {key: np.repeat(sc[key][behind:behind + 1], P, 0) for key in keys}
        a = pr.make_acc(P, 642, True)                             # (records of culled rows: to be ignored)
        src = np.arange(len(rows_at)) if len(rows_at) == 64 else np.array([3, 17, 40, 63])
        for key in keys:
            arrays[key][rows_at] = sc[key][src]
        a[rows_at] = acc[src]
        got = Run(sc, a, arrays=arrays).got()
        bad = []
        for key, val in got.items():
            if val is not None:
                x, y = val.reshape(P, -1)[rows_at], base[key].reshape(64, -1)[src]
                diff = np.nonzero((x != y).any(1))[0]
                if len(diff):
                    rel = np.abs(x[diff].astype(np.float64) - y[diff]).max(1) / np.abs(y[diff]).max(1)
                    bad.append(f"{key}: {len(diff)} rows differ (Gaussians {src[diff][:6].tolist()}.. at rows {rows_at[diff][:6].tolist()}.. of {P}), "
                               f"by up to {rel.max():.2e} of the row's largest element")
                rest = np.delete(val.reshape(P, -1), rows_at, 0)
                assert np.all(rest == 0), f"{key}: a culled filler row is not zero"
        return bad
    bad = place(np.arange(37, 101), 101) + place(np.array([0, 64, 128, 192]), 256)
    print("[preprocess-alone] layout: " + ("every row bit for bit" if not bad else "; ".join(bad)))
    assert not bad, bad


def test_worst_ratios_over_the_rows():
    """Runs last in this file: the worst row per output and class over the rows above, as a multiple of the class's e32."""
    print("[preprocess-alone] device, worst ratio per output and class (x e32):\n" + pr.worst_table("device"))
    assert pr.WORST and max(pr.WORST.values()) <= pr.MARGIN
