"""The per-Gaussian headers (d3ga_math.h, raster_pre_body.h) compiled for the host, alone against float64 on the edge scenes of
tests/preprocess_ref.py: per-row bars of 4 e32 where tests/test_hostcheck_math.py holds one global 1e-3 per tensor, culled rows in
the single-view backward, the guard band in x, in y and in both.  Runs without a GPU; it is also where the scene builder and the
bars prove themselves before tests/test_gpu_preprocess_alone.py spends GPU time on them.

Measured on this build (g++ -O2 -ffp-contract=off), worst row over the cases below, as a multiple of e32: docs/LOG.md,
"Per-Gaussian kernels alone against float64"."""
import ctypes

import numpy as np
import pytest

import preprocess_ref as pr
from conftest import ptr
from d3ga_amd._lib import RasterParams

P_HOST = 129

# id, Cfg arguments, inverse depth in acc, use_dcol
CASES = [
    ("sh16_deg0_cov6", dict(M=16, deg=0), False, 0),
    ("sh16_deg1_sr1", dict(M=16, deg=1, from_sr=True, mod=1.0), True, 1),
    ("sh16_deg2_sr13", dict(M=16, deg=2, from_sr=True, mod=1.3), False, 0),
    ("sh16_deg3_cov6", dict(M=16, deg=3), True, 0),
    ("sh16_deg3_cov6_dcol", dict(M=16, deg=3), True, 1),
    ("sh9_deg2_cov6", dict(M=9, deg=2), False, 0),
    ("sh4_deg1_sr13", dict(M=4, deg=1, from_sr=True, mod=1.3), True, 1),
    ("sh1_deg0_sr1", dict(M=1, deg=0, from_sr=True, mod=1.0), False, 0),
    ("colours_cov6", dict(M=0, deg=0), True, 0),
    ("colours_sr13", dict(M=0, deg=0, from_sr=True, mod=1.3), False, 0),
    ("aa_invdepth_sh16_deg3_cov6", dict(M=16, deg=3, aa=True), True, 1),
    ("aa_invdepth_sh16_deg2_sr13", dict(M=16, deg=2, from_sr=True, mod=1.3, aa=True), True, 0),
    ("aa_invdepth_colours_sr1", dict(M=0, deg=0, from_sr=True, mod=1.0, aa=True), True, 0),
    ("aa_invdepth_colours_cov6", dict(M=0, deg=0, aa=True), True, 0),
]


def host_prm(cfg, P):
    return RasterParams(P=P, M=cfg.M, sh_degree=cfg.deg, W=cfg.W, H=cfg.H, tanfovx=cfg.tanx, tanfovy=cfg.tany, scale_modifier=cfg.mod,
                        antialiasing=int(cfg.aa), prefiltered=0, debug=0)


def host_forward(hostcheck, sc, cfg):
    P, prm = sc["P"], host_prm(cfg, sc["P"])
    view, proj, campos = pr.cam_arrays(sc["cams"][0])
    shs = np.ascontiguousarray(sc["shs"][:, :cfg.M]) if cfg.sh else None
    o = dict(depth=np.zeros(P, np.float32), xy=np.zeros((P, 2), np.float32), conic_o=np.zeros((P, 4), np.float32),
             rgb=np.zeros((P, 3), np.float32), radii=np.zeros(P, np.int32), rect=np.zeros((P, 4), np.int32),
             clamped=np.zeros(P, np.uint8), cov3D=np.zeros((P, 6), np.float32))
    hostcheck.hc_preprocess(ctypes.byref(prm), ptr(sc["means3D"]), ptr(shs), ptr(None if cfg.sh else sc["rgb"]), ptr(sc["opacities"]),
                            ptr(sc["scales"] if cfg.from_sr else None), ptr(sc["rotations"] if cfg.from_sr else None),
                            ptr(None if cfg.from_sr else sc["cov6"]), ptr(view), ptr(proj), ptr(campos), ptr(o["depth"]), ptr(o["xy"]),
                            ptr(o["conic_o"]), ptr(o["rgb"]), ptr(o["radii"]), ptr(o["rect"]), ptr(o["clamped"]), ptr(o["cov3D"]))
    return o


def host_backward(hostcheck, sc, cfg, fwd, acc, use_dcol):
    P, prm = sc["P"], host_prm(cfg, sc["P"])
    view, proj, campos = pr.cam_arrays(sc["cams"][0])
    shs = np.ascontiguousarray(sc["shs"][:, :cfg.M]) if cfg.sh else None
    z = lambda *s: np.full(s, np.nan, np.float32)                   # every element must be written
    g = dict(means3D=z(P, 3), m2=z(P, 3), opacities=z(P, 1), sh=z(P, cfg.M, 3) if cfg.sh else None, colors=None if cfg.sh else z(P, 3),
             cov3D=None if cfg.from_sr else z(P, 6), scales=z(P, 3) if cfg.from_sr else None, rotations=z(P, 4) if cfg.from_sr else None)
    hostcheck.hc_preprocess_bwd(ctypes.byref(prm), ptr(sc["means3D"]), ptr(shs), ptr(sc["scales"] if cfg.from_sr else None),
                                ptr(sc["rotations"] if cfg.from_sr else None), ptr(view), ptr(proj), ptr(campos), ptr(fwd["radii"]),
                                ptr(fwd["cov3D"]), ptr(fwd["clamped"]), ptr(acc), ptr(g["means3D"]), ptr(g["m2"]), ptr(g["opacities"]),
                                ptr(g["sh"]), ptr(g["colors"]), ptr(g["cov3D"]), ptr(g["scales"]), ptr(g["rotations"]),
                                ptr(np.ascontiguousarray(fwd["conic_o"][:, 3])), int(use_dcol))
    return g


def test_the_table_reaches_every_class_at_every_size():
    """The rows of the class table for the sizes the tests use: a scene with room for the table holds all of it, a smaller one every
    class it has room for."""
    assert pr.TABLE_ROWS == 68 and len(pr.table_kinds(257)) == 68
    for cls, kinds, counts in pr.CLASS_TABLE:
        assert sum(counts) >= 8, cls
    assert {pr.KIND_CLASS[k] for k in pr.table_kinds(65)} == {c for c, _, _ in pr.CLASS_TABLE}
    assert len(set(pr.table_kinds(65))) >= 20 and pr.table_kinds(1) == ["plain_axis"]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_edge_scene_alone_against_float64(hostcheck, case):
    name, kw, invdepth, use_dcol = case
    cfg = pr.Cfg(**kw)
    sc = pr.edge_scene(P_HOST, 100 + CASES.index(case), cfg)
    counts = pr.assert_classes(sc)
    print(f"[preprocess-alone] host {name}: classes {counts}")
    acc = pr.make_acc(P_HOST, 7 + CASES.index(case), invdepth)
    ref64, ref32 = pr.reference(sc, cfg, acc, pr.torch.float64), pr.references32(sc, cfg, acc)
    e32 = pr.bars(ref64, ref32, sc)
    fwd = host_forward(hostcheck, sc, cfg)
    np.testing.assert_array_equal(fwd["radii"], ref64["radii"])
    vis = ref64["vis"]
    if cfg.sh:
        mask = (fwd["clamped"][:, None] >> np.arange(3)[None]) & 1
        np.testing.assert_array_equal(mask[vis].astype(bool), ref64["clamped"][vis])
    got = host_backward(hostcheck, sc, cfg, fwd, acc, use_dcol)
    pr.check_grads(got, ref64, e32, sc, cfg, acc, f"host {name}", m2=got["m2"])


def test_worst_ratios_over_the_cases():
    """Runs last in this file: the worst row per output and class over the cases above, as a multiple of the class's e32."""
    print("[preprocess-alone] host, worst ratio per output and class (x e32):\n" + pr.worst_table("host"))
    assert pr.WORST and max(pr.WORST.values()) <= pr.MARGIN
