"""Point location and the 3-NN scale seed (d3ga_amd/tetra.py, csrc/bary.hip) without a GPU: the g++ build of csrc/bary_math.h
(tests/hostcheck/locatecheck.cpp, -ffp-contract=off as the device build) against the float64 oracles of tests/locate_ref.py on
every case and both routes, the stand-alone program under the sanitizers, the status codes of the entry points for arguments
refused before any HIP call, and builds of the same text with one rule broken, which the cases must notice."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import locate_ref as lr
from conftest import ROOT


def test_host_build_equals_the_oracle():
    """Every case through the exhaustive and the grid route of the g++ build: the oracle's protocol (locate_ref.check_bary), the
    two routes bit for bit, cases that restate another reproduce it bit for bit.  Prints what locate_ref.MEASURED and
    MARGINAL_SHARES record and holds the host build to BARS / 8."""
    worst = 0.0
    for name in lr.CASES:
        c = lr.case(name)
        b_e, t_e, a_e = lr.host_compute_bary(name, "exhaustive")
        b_g, t_g, a_g = lr.host_compute_bary(name, "grid")
        assert np.array_equal(lr.bits(b_e), lr.bits(b_g)) and np.array_equal(t_e, t_g) and np.array_equal(a_e, a_g), f"{name}: grid != exhaustive"
        if name in ("dyadic4", "dyadic4_perm", "jitter_T1"):               # the lists of the grid in descending order: the same
            b_r, t_r, a_r = lr.host_compute_bary(name, "grid_reversed")
            assert np.array_equal(lr.bits(b_e), lr.bits(b_r)) and np.array_equal(t_e, t_r) and np.array_equal(a_e, a_r), f"{name}: grid, lists reversed"
        err = lr.check_bary(name, b_e, t_e, a_e)
        if "same_as" in c:
            b0, t0, a0 = lr.host_compute_bary(c["same_as"], "exhaustive")
            keep = np.ones(len(t0), bool)
            keep[c.get("bad_rows", [])] = False
            assert np.array_equal(lr.bits(b_e)[keep], lr.bits(b0)[keep]) and np.array_equal(t_e[keep], t0[keep]) and np.array_equal(a_e[keep], a0[keep]), \
                f"{name}: differs from {c['same_as']}"
        if not c["exact"]:
            worst = max(worst, err)
            free, every = lr.marginal_share(name)
            print(f"{name}: max |w_host - w_f64| = {err:.3g}; marginal {free:.4f} of the queries not placed on a face ({every:.4f} of all)")
            assert free <= lr.MARGINAL_CAP, (name, free)
            if name in lr.MARGINAL_SHARES:
                assert lr.MARGINAL_SHARES[name] == (round(free, 4), round(every, 4)), (name, free, every)
    print(f"MEASURED bary = {worst:.3g}; BARS = {8 * worst:.3g}")
    assert worst <= lr.MEASURED["bary"], worst
    assert worst >= lr.MEASURED["bary"] / 2, f"MEASURED is stale: {worst}"
    assert set(lr.MARGINAL_SHARES) == {n for n in lr.CASES if not lr.case(n)["exact"]}


def test_the_dyadic_cases_hold_what_they_are_there_for():
    """dyadic4: exact ties for the best tet on most points, up to 24 tets tied, winners on both sides of tet 256, active at a
    minimum weight of exactly 0, points outside; dyadic4_perm: ties that straddle 255 | 256."""
    from oracle import bary as ob
    c, ref = lr.case("dyadic4"), lr.oracle("dyadic4")
    assert c["corners"].shape[0] == 384 and c["points"].shape[0] == 6859
    tie = ref["m1"] == ref["m2"]
    assert 0.84 < tie.mean() < 0.85 and 0.71 < ref["active"].mean() < 0.72
    assert (ref["m1"] == 0).sum() > 1000 and ref["active"][ref["m1"] == 0].all()
    assert (ref["tid"] < 256).any() and (ref["tid"] >= 256).any()
    for name in ("dyadic4", "dyadic4_perm"):
        c, ref = lr.case(name), lr.oracle(name)
        a, b, cc, d = (c["corners"].astype(np.float64)[None, :, k] for k in range(4))
        straddle, most = 0, 0
        for s in range(0, 6859, 512):
            mn = ob.barycentric(a, b, cc, d, c["points"][s:s + 512, None, :].astype(np.float64)).min(-1)
            tied = mn == ref["m1"][s:s + 512, None]
            most = max(most, int(tied.sum(1).max()))
            straddle += int((tied[:, :256].any(1) & tied[:, 256:].any(1)).sum())
        assert most == 24 and straddle > 100, (name, most, straddle)


def test_degenerate_tets_are_never_chosen():
    """Every tet degenerate -> (0, 0, False) by both routes; the flat tets of `flat_members` have a float32 volume of exactly 0
    (that they would capture queries if they competed is what the mutation `zero_volume_tets_compete` below shows)."""
    flat = lr.flat_tets(lr.case("jitter_T1")["points"], 640)
    assert flat.shape == (32, 4, 3) and (lr.vol6_f32(flat) == 0).all()
    pts = lr.case("jitter_T1")["points"][:300]
    many = np.concatenate([flat, flat, flat])                              # 96 tets: the grid route
    for method in ("exhaustive", "grid"):
        for tets in (flat, many):
            b, t, a = lr.host_compute_bary_arrays(pts, tets, method)
            assert (lr.bits(b) == 0).all() and (t == 0).all() and not a.any()


def test_knn3_host_build_equals_the_brute_force():
    """Every cloud through the exhaustive loop and the ring search of the g++ build: within the bar of the float64 brute force,
    exactly the float32 value on the dyadic clouds, the two routes bit for bit."""
    for name in lr.KNN_CASES:
        e, g = lr.host_knn(name, "exhaustive"), lr.host_knn(name, "grid")
        assert np.array_equal(lr.bits(e), lr.bits(g)), f"{name}: ring search != exhaustive"
        worst = lr.check_knn(name, e)
        print(f"{name}: P = {e.shape[0]}, largest error {worst:.3f} of the bar")
        assert worst <= 1.0, (name, worst)
    p, _ = lr.knn_case("uniform2")
    d = ((p[0].astype(np.float64) - p[1].astype(np.float64)) ** 2).sum()
    np.testing.assert_allclose(lr.host_knn("uniform2"), [d / 3, d / 3], rtol=lr.KNN_REL)
    assert lr.host_knn("uniform1")[0] == 0.0


def test_knn3_grid_of_the_cases_is_what_they_are_there_for():
    from d3ga_amd.tetra import _point_grid
    dims = lambda name: list(_point_grid(torch.from_numpy(lr.knn_case(name)[0].copy()))[3])
    assert lr.knn_case("lattice16x16x8")[0].shape[0] == 2048
    assert dims("planar47") == [257, 257, 1]
    _, _, origin_h, d = _point_grid(torch.from_numpy(lr.knn_case("planar257x9")[0].copy()))
    assert abs(origin_h[3] - 0.1) < 1e-6
    start, _, _, d = _point_grid(torch.from_numpy(lr.knn_case("outlier")[0].copy()))
    assert int(np.diff(start.numpy()).max()) >= 2400               # nearly every point in one cell


def test_knn3_coordinates_that_are_not_finite():
    """The grid builder refuses them with a ValueError that says so; the exhaustive loop gives the bad row 0 and leaves every
    other row as it is without that point's distances."""
    from d3ga_amd.tetra import _point_grid
    p = lr.knn_case("uniform2049")[0].copy()
    for bad in (np.nan, np.inf, -np.inf):
        q = p.copy()
        q[100, 1] = bad
        with pytest.raises(ValueError, match="knn_mean_dist2: points hold coordinates that are not finite"):
            _point_grid(torch.from_numpy(q))
        out = lr.host_knn_arrays(q, "exhaustive")
        rest = np.delete(np.arange(len(p)), 100)
        assert out[100] == 0.0 and np.array_equal(lr.bits(out[rest]), lr.bits(lr.host_knn_arrays(p[rest], "exhaustive")))


def test_locatecheck_under_the_sanitizers(tmp_path):
    """The stand-alone program of tests/hostcheck/locatecheck.cpp: both searches of both helpers on a built-in cage with exact
    ties, outside points, zero-volume tets and points that are not finite."""
    exe = str(tmp_path / "locatecheck")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DLOCATECHECK_MAIN", lr.HOSTCHECK_SRC, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "locatecheck: ok", (out.stdout, out.stderr[-2000:])


def test_entry_points_refuse_bad_arguments_no_gpu_needed():
    """The status table of the four entry points of bary.hip for arguments refused before any HIP call: every pointer below is
    a made-up non-NULL address that is never read (origin_h and dims are HOST arrays and real)."""
    import d3ga_amd
    from d3ga_amd.csrc import build as b
    L = d3ga_amd.lib()
    OK, E_NULL, E_SIZE, E_CONFIG = 0, -1, -2, -3
    p, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)
    origin_h, dims = (ctypes.c_float * 4)(0, 0, 0, 0.5), (ctypes.c_int32 * 3)(2, 2, 2)
    assert L.d3ga_compute_bary(-1, 4, p, p, p, p, p, None) == E_SIZE and L.d3ga_compute_bary(4, 0, p, p, p, p, p, None) == E_SIZE
    assert L.d3ga_compute_bary(0, 4, None, None, None, None, None, None) == OK
    for k in range(5):
        args = [p] * 5
        args[k] = None
        assert L.d3ga_compute_bary(4, 4, *args, None) == E_NULL
    assert L.d3ga_compute_bary(4, 4, p, p, odd, p, p, None) == E_CONFIG           # barys is stored as float4
    assert L.d3ga_compute_bary(4, 4, p, p, ctypes.c_void_p(0x1008), p, p, None) == E_CONFIG
    grid = lambda P=4, barys=p, o=origin_h, d=dims, pts=p: L.d3ga_compute_bary_grid(P, pts, p, p, p, o, d, barys, p, p, None)
    assert grid(P=-1) == E_SIZE and grid(P=0) == OK and grid(pts=None) == E_NULL and grid(barys=None) == E_NULL
    assert grid(d=(ctypes.c_int32 * 3)(2, 0, 2)) == E_SIZE and grid(o=(ctypes.c_float * 4)(0, 0, 0, 0)) == E_SIZE
    assert grid(o=(ctypes.c_float * 4)(0, 0, 0, float("nan"))) == E_SIZE
    assert grid(barys=odd) == E_CONFIG
    assert L.d3ga_knn3_mean_dist2(-1, p, p, None) == E_SIZE and L.d3ga_knn3_mean_dist2(0, None, None, None) == OK
    assert L.d3ga_knn3_mean_dist2(4, None, p, None) == E_NULL and L.d3ga_knn3_mean_dist2(4, p, None, None) == E_NULL
    kgrid = lambda P=4, out=p, o=origin_h, d=dims: L.d3ga_knn3_mean_dist2_grid(P, p, p, p, o, d, out, None)
    assert kgrid(P=-1) == E_SIZE and kgrid(P=0) == OK and kgrid(out=None) == E_NULL
    assert kgrid(d=(ctypes.c_int32 * 3)(0, 1, 1)) == E_SIZE and kgrid(o=(ctypes.c_float * 4)(0, 0, 0, -1)) == E_SIZE
    # the device build is the host build's twin: the header is a dependency and contraction is off
    assert "bary_math.h" in b.HEADERS and "-ffp-contract=off" in b.EXTRA["bary.hip"] and "-fhip-fp32-correctly-rounded-divide-sqrt" in b.EXTRA["bary.hip"]


# One rule of csrc/bary_math.h broken at a time: (text, replacement, the cases of which at least one must notice)
MUTATIONS = {
    "exhaustive_ties_take_the_last": ("if (tw.mn > b.mn) bary_best_take(b, tw, t);", "if (tw.mn >= b.mn) bary_best_take(b, tw, t);", ("dyadic4",)),
    "grid_ties_ignore_the_index": ("if (tw.mn > b.mn || (tw.mn == b.mn && t < b.t)) bary_best_take(b, tw, t);", "if (tw.mn > b.mn) bary_best_take(b, tw, t);",
                                   ("dyadic4", "dyadic4_perm")),
    "chunk_drops_its_last_tet": ("for (int j = 0; j < cnt; ++j) bary_select_exhaustive", "for (int j = 0; j < cnt - (cnt == kBaryChunk); ++j) bary_select_exhaustive",
                                 ("one_each_256",)),
    "zero_volume_tets_compete": ("if (vol6 == 0.f || !finite) r.mn = -INFINITY;", "", ("flat_members",)),
}


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_the_cases_notice_a_broken_rule(mutation, tmp_path):
    """The same hostcheck source over a copy of the header with one rule broken: the case written for that rule fails."""
    old, new, cases = MUTATIONS[mutation]
    csrc = tmp_path / "d3ga_amd" / "csrc"
    host = tmp_path / "tests" / "hostcheck"
    csrc.mkdir(parents=True)
    host.mkdir(parents=True)
    text = open(os.path.join(ROOT, "d3ga_amd", "csrc", "bary_math.h")).read()
    assert text.count(old) == 1, mutation
    (csrc / "bary_math.h").write_text(text.replace(old, new))
    for h in ("d3ga_math.h", "knn_math.h"):
        shutil.copy(os.path.join(ROOT, "d3ga_amd", "csrc", h), csrc / h)
    shutil.copy(lr.HOSTCHECK_SRC, host / "locatecheck.cpp")
    so = str(tmp_path / "libbroken.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", str(host / "locatecheck.cpp"), "-o", so])
    broken = ctypes.CDLL(so)
    noticed = []
    for name in cases:
        c = lr.case(name)
        for method in ("exhaustive", "grid", "grid_reversed"):
            res = lr.host_compute_bary_arrays(c["points"], c["corners"], method, lib=broken)
            try:
                lr.check_bary(name, *res)
                want = lr.host_compute_bary(c.get("same_as", name), "exhaustive")
                assert all(np.array_equal(x, y) for x, y in zip(res, want))
            except AssertionError:
                noticed.append((name, method))
    assert noticed, f"{mutation}: no case noticed"
