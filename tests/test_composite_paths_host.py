"""CPU checks behind tests/test_gpu_composite_paths.py: the path tables reach every instantiation of the compositing kernels and
every feasible pair of factor values, the Python mirror of the two dispatches behaves as the dispatch code reads, and the scenes
have the properties the GPU rows rely on -- all from tests/composite_ref.py and the C oracle, no GPU."""
import numpy as np

import composite_ref as ref

FWD_ROWS, BWD_ROWS = ref.fwd_table(), ref.bwd_table()


def test_instance_sets_are_the_full_products():
    assert len(ref.ALL_FWD_INSTANCES) == 24 and len(ref.ALL_BWD_INSTANCES) == 24
    assert {i[0] for i in ref.ALL_FWD_INSTANCES} == {"plain", "pair", "l1"} and {i[0] for i in ref.ALL_BWD_INSTANCES} == {"plain", "pair", "depth"}
    assert {i[1] for i in ref.ALL_BWD_INSTANCES} == {256, 512}


def test_dispatch_mirror():
    """The refusals of the two dispatches, per_view_background without a batch, and the cache size on either side of 512."""
    assert ref.fwd_instance(True, True, False, 1, False, False) is None
    assert ref.bwd_instance(True, True, 512, 1, False, False) is None
    assert ref.fwd_instance(False, False, True, 1, True, True) == ("plain", True, False, True)         # one view: bg is (3,)
    assert ref.fwd_instance(True, False, False, 2, True, False) == ("pair", False, True, False)
    assert ref.bwd_instance(False, True, 511, 2, True, True) == ("depth", 256, True, True)
    assert ref.bwd_instance(False, False, 512, 0, True, False) == ("plain", 512, False, False)
    assert ref.bwd_instance(True, False, 1024, 2, False, True) == ("pair", 512, False, True)


def test_forward_rows_reach_every_instantiation_and_pair():
    assert {r["inst"] for r in FWD_ROWS} == ref.ALL_FWD_INSTANCES
    assert all(r["inst"] == ref.row_fwd_instance(r) for r in FWD_ROWS)
    assert ref.pairs_missing(FWD_ROWS, ref.FWD_FACTORS, ref.fwd_feasible) == []
    assert len({r["id"] for r in FWD_ROWS}) == len(FWD_ROWS) <= 48
    assert {r["k"] for r in FWD_ROWS if not r["pvb"]} == {1, 2}, "a shared background over two views"
    assert all(r["k"] == 2 for r in FWD_ROWS if r["pvb"])


def test_backward_rows_reach_every_instantiation_and_pair():
    assert {r["inst"] for r in BWD_ROWS} == ref.ALL_BWD_INSTANCES
    assert all(r["inst"] == ref.row_bwd_instance(r) for r in BWD_ROWS)
    assert ref.pairs_missing(BWD_ROWS, ref.BWD_FACTORS, ref.bwd_feasible) == []
    assert len({r["id"] for r in BWD_ROWS}) == len(BWD_ROWS) <= 72
    # the six inverse-depth instantiations of a batch or a window, and the gradient forms without dL_dpix
    assert {r["inst"][2:] for r in BWD_ROWS if r["mode"] == "depth"} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {"l1t", "l1c", "invd"} <= {r["src"] for r in BWD_ROWS}
    deep = [r for r in BWD_ROWS if r["scene"] == "deep"]
    assert {r["slots"] for r in deep} == {256, 512} and {r["mode"] for r in deep} == {"plain", "pair", "depth"}
    assert {0, 1, 2} <= {r["assign"] for r in deep} and {0, 3} <= {r["split"] for r in deep}
    assert {(r["mode"], r["slots"]) for r in deep} == {(m, s) for m in ("plain", "pair", "depth") for s in (256, 512)}
    # bwd_split n > 0 acts only under the work order (bit 5 of composite_variant)
    assert any(r["split"] == 3 and r["variant"] & 32 for r in BWD_ROWS)


def test_infeasible_pairs_are_only_the_coupled_ones():
    """The feasibility rules drop nothing but mode x target (forward) and mode x src (backward)."""
    full = lambda f: sum(len(a) * len(b) for i, a in enumerate(f.values()) for b in list(f.values())[i + 1:])
    count = lambda f, ok: sum(ok(fa, a, fb, b) for i, (fa, va) in enumerate(f.items()) for fb, vb in list(f.items())[i + 1:] for a in va for b in vb)
    assert full(ref.FWD_FACTORS) - count(ref.FWD_FACTORS, ref.fwd_feasible) == 9 - 4          # 3 x 3 pairs, 4 of them exist
    assert full(ref.BWD_FACTORS) - count(ref.BWD_FACTORS, ref.bwd_feasible) == 21 - 8         # 3 x 7 pairs: plain 5, pair 1, depth 2


def test_small_scene_views():
    """600 Gaussians on 96 x 80 (6 x 5 tiles); the windowed views: 37 x 29 windows at offsets that are no multiple of 8, one at
    the left / bottom and one at the right / top of its padded raster."""
    (a, b) = ref.views("small2")
    assert (a.W, a.H, b.W, b.H) == (96, 80, 96, 80) and ref.gaussians("small")["means3D"].shape == (600, 3)
    assert not np.allclose(a.view, b.view)
    (c, d) = ref.views("smallw2")
    assert (c.W, c.H, d.W, d.H) == (37, 29, 37, 29)
    assert (c.ox == 0, c.oy == 0, d.ox == 0, d.oy == 0) == (True, False, False, True)
    assert c.oy % 8 and d.ox % 8 and (c.w, c.h) != (d.w, d.h)
    for name in ("small1", "small2", "smallw1", "smallw2"):
        for v in range(len(ref.views(name))):
            r = ref.render(name, v)
            assert float(np.abs(r.color - np.asarray(ref.BG0, np.float32)[:, None, None]).max()) > 0.05, "the window shows the avatar"
            assert r.pix.mean() <= 0.05


def test_l1_targets_keep_their_distance():
    for name, pvb in (("small1", False), ("small2", True), ("smallw2", True), ("deep1", False)):
        inc = ref.incoming(name, pvb)
        for v, r in enumerate(ref.row_renders(name, pvb)):
            assert (np.abs(r.color.astype(np.float64) - inc["target"][v]) >= 1e-3).all()
            assert not inc["gpix"][v][:, r.pix].any() and not inc["gd"][v][r.pix].any()


def test_deep_scene_preconditions():
    """Nothing saturates (no early termination), at most 5 % marginal pixels, and one tile holds >= 512 + 64 entries that blend on
    some pixel of it: at least 64 records of that tile must leave the 512-slot merge cache early (more at 256 slots)."""
    f = ref.deep_facts()
    print(f)
    assert f["P"] == 1400 and f["pixels"] == 1024 and len(f["lens"]) == 4
    assert f["min_T"] > 1e-3
    assert f["marginal"] <= 0.05 * f["pixels"]
    assert max(f["alive"]) >= 512 + 64, f["alive"]
    assert f["with_opacity_grad"] >= 0.95 * f["P"]
