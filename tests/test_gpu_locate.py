"""Point location (`tetra.compute_bary`) and the 3-NN scale seed (`tetra.knn_mean_dist2`) on the GPU, every route of both: against
the float64 oracles of tests/locate_ref.py (exactly on the dyadic cases, the margin protocol elsewhere), against the g++ build of
csrc/bary_math.h bit for bit (bary.hip is compiled without contraction and with correctly rounded division), grid against
exhaustive bit for bit, the raw entry points between guard bands, and what the Python layer does with inputs that are not
float32, contiguous and detached."""
import ctypes

import numpy as np
import pytest
import torch

import locate_ref as lr

pytestmark = pytest.mark.gpu
DEV = "cuda"
METHODS = ("exhaustive", "grid", None)                       # None: the default
GUARD = 64                                                   # words in front of and behind every output
NAN_BITS = 0x7FC0DEAD                                        # a pattern no kernel would produce


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)              # a copy: the cases are read-only arrays


def _np(*ts):
    out = tuple(t.detach().cpu().numpy() for t in ts)
    return out[0] if len(out) == 1 else out


def _locate(points, corners, method):
    from d3ga_amd.tetra import compute_bary
    kw = {} if method is None else {"method": method}
    barys, tid, active = compute_bary(_dev(points), _dev(corners), **kw)
    assert barys.dtype == torch.float32 and tid.dtype == torch.int64 and active.dtype == torch.bool
    assert not barys.requires_grad and barys.is_contiguous()
    return barys, tid, active


@pytest.mark.parametrize("name", lr.CASES)
def test_compute_bary_every_route(name):
    """exhaustive, grid and the default: the oracle's protocol, the host build bit for bit, the routes equal among themselves"""
    c = lr.case(name)
    host = lr.host_compute_bary(name, "exhaustive")
    first = None
    for method in METHODS:
        res = _locate(c["points"], c["corners"], method)
        barys, tid, active = _np(*res)
        err = lr.check_bary(name, barys, tid, active)
        print(f"{name} [{method}]: max |w - w_f64| = {err:.3g} (bar {lr.BARS['bary']:.3g})")
        assert err <= lr.BARS["bary"], (name, method, err)
        assert np.array_equal(lr.bits(barys), lr.bits(host[0])) and np.array_equal(tid, host[1]) and np.array_equal(active, host[2]), \
            f"{name} [{method}]: the device differs from the g++ build of bary_math.h"
        if first is None:
            first = res
        else:
            assert all(torch.equal(x, y) for x, y in zip(res, first)), f"{name}: {method} != exhaustive"
    if "same_as" in c:                                        # (implied by the host equalities; stated for the device on its own)
        b0, t0, a0 = _np(*_locate(lr.case(c["same_as"])["points"], lr.case(c["same_as"])["corners"], None))
        keep = np.ones(len(t0), bool)
        keep[c.get("bad_rows", [])] = False
        barys, tid, active = _np(*first)
        assert np.array_equal(lr.bits(barys)[keep], lr.bits(b0)[keep]) and np.array_equal(tid[keep], t0[keep]) and np.array_equal(active[keep], a0[keep])


def test_compute_bary_of_no_points_and_of_degenerate_tets_only():
    c = lr.case("dyadic4")
    flat = lr.flat_tets(lr.case("jitter_T1")["points"], 640)
    for method in METHODS:
        barys, tid, active = _locate(c["points"][:0], c["corners"], method)
        assert barys.shape == (0, 4) and tid.shape == (0,) and active.shape == (0,)
        for tets in (flat, np.concatenate([flat, flat, flat])):            # 32: the exhaustive route whatever the method; 96: the grid
            barys, tid, active = _locate(lr.case("jitter_T1")["points"][:300], tets, method)
            assert not barys.any() and not tid.any() and not active.any()


def test_compute_bary_inputs_are_detached_float32_contiguous_copies():
    c = lr.case("jitter_T1")
    want = _locate(c["points"][:700], c["corners"], None)
    from d3ga_amd.tetra import compute_bary
    p, t = _dev(c["points"][:700]), _dev(c["corners"])
    wide_p = torch.zeros((700, 5), device=DEV)
    wide_p[:, 1:4] = p
    wide_t = torch.zeros((t.shape[0], 4, 6), device=DEV)
    wide_t[:, :, ::2] = t
    variants = {"float64": (p.double(), t.double()), "strided": (wide_p[:, 1:4], wide_t[:, :, ::2]),
                "requires_grad": (p.clone().requires_grad_(True), t.clone().requires_grad_(True))}
    assert not variants["strided"][0].is_contiguous() and not variants["strided"][1].is_contiguous()
    for key, (pp, tt) in variants.items():
        for method in ("exhaustive", "grid"):
            got = compute_bary(pp, tt, method=method)
            assert all(torch.equal(x, y) for x, y in zip(got, want)), (key, method)
            assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64 and got[2].dtype == torch.bool
            assert not got[0].requires_grad and got[0].grad_fn is None, key


def _ulps(a, b):
    """the largest |a - b| in float32 ulps of the larger magnitude"""
    a, b = a.astype(np.float32), b.astype(np.float32)
    ulp = np.spacing(np.maximum(np.abs(a), np.abs(b)))
    return float((np.abs(a.astype(np.float64) - b.astype(np.float64)) / ulp).max()) if a.size else 0.0


@pytest.mark.parametrize("name", lr.KNN_CASES)
def test_knn_mean_dist2_every_route(name):
    """exhaustive, grid (the ring search from 2048 points) and the default: within the bar of the float64 brute force, the float32
    value on the dyadic clouds, the host build bit for bit, the routes equal; and knn_points(K = 4)'s mean of its last three"""
    from d3ga_amd.knn import knn_points
    from d3ga_amd.tetra import knn_mean_dist2
    p = _dev(lr.knn_case(name)[0])
    host = lr.host_knn(name, "exhaustive")
    first = None
    for method in METHODS:
        out = knn_mean_dist2(p, **({} if method is None else {"method": method}))
        assert out.dtype == torch.float32 and out.shape == (p.shape[0],) and not out.requires_grad
        worst = lr.check_knn(name, _np(out))
        print(f"{name} [{method}]: largest error {worst:.3f} of the bar")
        assert worst <= 1.0, (name, method, worst)
        assert np.array_equal(lr.bits(_np(out)), lr.bits(host)), f"{name} [{method}]: the device differs from the g++ build"
        first = out if first is None else first
        assert torch.equal(out, first), (name, method)
    same = knn_points(p[None], p[None], K=4).dists[0, :, 1:].mean(-1)
    ulps = _ulps(_np(same), _np(first))
    print(f"{name}: knn_points(K=4)[:, 1:].mean(-1) within {ulps:.2f} ulps")
    assert ulps <= 2.0, (name, ulps)


def test_knn_mean_dist2_names_and_inputs():
    import os
    import sys
    from conftest import ROOT
    from d3ga_amd.tetra import knn_mean_dist2
    sys.path.insert(0, os.path.join(ROOT, "compat"))          # INTEGRATION.md sec. 1 puts compat/ on sys.path
    try:
        from simple_knn._C import distCUDA2                   # models/mesh_net.py:22
    finally:
        sys.path.remove(os.path.join(ROOT, "compat"))
    pts = lr.knn_case("uniform2049")[0]
    p = _dev(pts)
    want = knn_mean_dist2(p)
    assert torch.equal(distCUDA2(p), want)
    wide = torch.zeros((p.shape[0], 4), device=DEV)
    wide[:, :3] = p
    for key, q in {"float64": p.double(), "strided": wide[:, :3], "requires_grad": p.clone().requires_grad_(True)}.items():
        for method in ("exhaustive", "grid"):
            out = knn_mean_dist2(q, method=method)
            assert torch.equal(out, want) and out.dtype == torch.float32 and not out.requires_grad and out.grad_fn is None, (key, method)
    assert knn_mean_dist2(p[:0]).shape == (0,) and knn_mean_dist2(p[:0], method="exhaustive").dtype == torch.float32


def test_knn_mean_dist2_coordinates_that_are_not_finite():
    """From 2048 points the grid route refuses them with a ValueError that says so; the exhaustive kernel (below 2048 points, or
    asked for) gives the bad row 0 and leaves every other row as it is without that point."""
    from d3ga_amd.tetra import knn_mean_dist2
    pts = lr.knn_case("uniform2049")[0]
    for bad in (np.nan, np.inf, -np.inf):
        q = pts.copy()
        q[100, 1] = bad
        for kw in ({}, {"method": "grid"}):
            with pytest.raises(ValueError, match="knn_mean_dist2: points hold coordinates that are not finite"):
                knn_mean_dist2(_dev(q), **kw)
        rest = np.delete(np.arange(len(q)), 100)
        for n, kw in ((len(q), {"method": "exhaustive"}), (2047, {}), (2047, {"method": "grid"})):
            out = knn_mean_dist2(_dev(q[:n]), **kw)
            clean = knn_mean_dist2(_dev(q[:n][rest[rest < n]]), method="exhaustive")
            assert float(out[100]) == 0.0 and torch.equal(out[_dev(rest[rest < n])], clean), (bad, n, kw)


def _guarded(bufs, key, shape, dtype):
    """an output of `shape` between GUARD words of NAN_BITS on both sides (and up to the next word behind a byte tensor)"""
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    raw = torch.full(((nbytes + 3) // 4 + 2 * GUARD,), NAN_BITS, dtype=torch.int32, device=DEV)
    bufs[key] = (raw, nbytes)
    return raw.view(torch.uint8)[4 * GUARD:4 * GUARD + nbytes].view(dtype).view(shape)


def _guards_intact(bufs, tag):
    for key, (raw, nbytes) in bufs.items():
        fresh = torch.full_like(raw, NAN_BITS).view(torch.uint8)
        got = raw.view(torch.uint8)
        assert torch.equal(got[:4 * GUARD], fresh[:4 * GUARD]) and torch.equal(got[4 * GUARD + nbytes:], fresh[4 * GUARD + nbytes:]), (tag, key)
        if key == "active":
            assert bool((got[4 * GUARD:4 * GUARD + nbytes] <= 1).all()), (tag, key)
        else:
            assert not bool((raw[GUARD:GUARD + nbytes // 4] == NAN_BITS).any()), (tag, key)


@pytest.mark.parametrize("P", (257, 513))
def test_raw_entry_points_write_every_element_and_nothing_else(P):
    """d3ga_compute_bary, d3ga_compute_bary_grid (the lists of the grid ascending and descending), d3ga_knn3_mean_dist2 and
    d3ga_knn3_mean_dist2_grid at sizes that end inside a workgroup: every output between guard bands, results those of the
    host build."""
    from d3ga_amd import _lib
    from d3ga_amd.tetra import _point_grid, _tet_grid
    L, s = _lib.lib(), _lib.stream_handle()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    c = lr.case("dyadic4")
    pick = np.random.default_rng(P).permutation(c["points"].shape[0])[:P]           # inside, outside and tied points alike
    pts, cor = _dev(c["points"][pick]), _dev(c["corners"])
    T = cor.shape[0]
    host = lr.host_compute_bary("dyadic4", "exhaustive")
    bufs = {}
    barys, tid, active = _guarded(bufs, "barys", (P, 4), torch.float32), _guarded(bufs, "tid", (P,), torch.int32), _guarded(bufs, "active", (P,), torch.uint8)
    assert L.d3ga_compute_bary(P, T, ptr(pts), ptr(cor), ptr(barys), ptr(tid), ptr(active), s) == 0
    torch.cuda.synchronize()
    _guards_intact(bufs, "d3ga_compute_bary")
    assert np.array_equal(lr.bits(_np(barys)), lr.bits(host[0][pick])) and np.array_equal(_np(tid), host[1][pick]) and np.array_equal(_np(active) != 0, host[2][pick])
    start, items, origin_h, dims = _tet_grid(cor)
    for tag, lists in (("ascending", items), ("descending", _dev(lr.reverse_lists(_np(start), _np(items))))):
        bufs = {}
        b2, t2, mw = _guarded(bufs, "barys", (P, 4), torch.float32), _guarded(bufs, "tid", (P,), torch.int32), _guarded(bufs, "minw", (P,), torch.float32)
        assert L.d3ga_compute_bary_grid(P, ptr(pts), ptr(cor), ptr(start), ptr(lists), origin_h, dims, ptr(b2), ptr(t2), ptr(mw), s) == 0
        torch.cuda.synchronize()
        _guards_intact(bufs, "d3ga_compute_bary_grid " + tag)
        inside = host[2][pick]                                # a point inside is found by the grid alone, with the same tet and weights
        assert np.array_equal(_np(mw) >= 0, inside), tag
        assert np.array_equal(lr.bits(_np(b2))[inside], lr.bits(host[0][pick])[inside]) and np.array_equal(_np(t2)[inside], host[1][pick][inside]), tag
    cloud = lr.knn_case("duplicates")[0][:P]
    q = _dev(cloud)
    want = lr.host_knn_arrays(cloud, "exhaustive")
    bufs = {}
    out = _guarded(bufs, "out", (P,), torch.float32)
    assert L.d3ga_knn3_mean_dist2(P, ptr(q), ptr(out), s) == 0
    torch.cuda.synchronize()
    _guards_intact(bufs, "d3ga_knn3_mean_dist2")
    assert np.array_equal(lr.bits(_np(out)), lr.bits(want))
    start, items, origin_h, dims = _point_grid(q)
    bufs = {}
    out = _guarded(bufs, "out", (P,), torch.float32)
    assert L.d3ga_knn3_mean_dist2_grid(P, ptr(q), ptr(start), ptr(items), origin_h, dims, ptr(out), s) == 0
    torch.cuda.synchronize()
    _guards_intact(bufs, "d3ga_knn3_mean_dist2_grid")
    assert np.array_equal(lr.bits(_np(out)), lr.bits(want))
