"""The float64 oracle of knn_points, the inputs of its tests, and the g++ build of csrc/knn_math.h
(tests/hostcheck/knncheck.cpp) both test modules run.

The oracle is a brute force over every (query, point) pair: float64 squared distances of the float32 coordinates, a stable sort
(so equal distances -- identical points -- come lower index first), the K + 1 nearest of every query.  It flags the MARGINAL rows
no float32 implementation can be held to: two adjacent distances among the K + 1 nearest differ by less than GAP relative and
do not belong to identical points (then every implementation computes the same distance for both and the tie rule decides,
which is held exactly).  Away from the marginal rows idx must be exactly the oracle's; on them no chosen neighbour may be
farther than the oracle's K-th distance by more than GAP relative.  dists stay within 4 * 2^-24 d + 2^-149 of the float64
distance of the neighbour they name: three products and two additions, each with half an ulp (knn_dist2 makes up for the
rounding of its three subtractions, which that budget does not hold, at the price of one more addition).
"""
import ctypes
import os
import subprocess

import numpy as np

from conftest import ROOT

GAP = 2.0 ** -20
MARGINAL_CAP = 0.01          # of the rows, in every case
DIST_REL, DIST_ABS = 4 * 2.0 ** -24, 2.0 ** -149


def _uniform(P, seed, lo=0.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, (P, 3)).astype(np.float32)


def _self(P, seed, K):
    p = _uniform(P, seed)
    return dict(p1=p[None], p2=p[None], K=K)


def _outside():
    """257 queries against 1000 other points; every third query outside p2's bounding box, by up to two box sizes"""
    p2 = _uniform(1000, 21)
    q = _uniform(257, 22)
    rng = np.random.default_rng(23)
    lo, hi = p2.min(0), p2.max(0)
    for i in range(0, 257, 3):
        axis = rng.integers(0, 3)
        sign = rng.choice([-1.0, 1.0])
        far = rng.uniform(0.0, 2.0) * (hi - lo)[axis]
        q[i, axis] = (hi[axis] + far) if sign > 0 else (lo[axis] - far)
        if i % 2 == 0:                                         # and off along a second axis as well
            q[i, (axis + 1) % 3] = hi[(axis + 1) % 3] + rng.uniform(0.0, 2.0) * (hi - lo)[(axis + 1) % 3]
    return dict(p1=q.astype(np.float32)[None], p2=p2[None], K=4)


def _twice():
    p = _uniform(200, 31)
    both = np.concatenate([p, p])
    return dict(p1=both[None], p2=both[None], K=4)


def _flat():
    p = _uniform(1500, 41)
    p[:, 2] = np.float32(0.375)
    return dict(p1=p[None], p2=p[None], K=4)


def _batch2():
    a, b = _uniform(400, 51), _uniform(400, 52, -2.0, 3.0)
    q = np.stack([_uniform(130, 53), _uniform(130, 54, -2.0, 3.0)])
    return dict(p1=q, p2=np.stack([a, b]), K=4)


BUILDERS = {
    "self300_K4": lambda: _self(300, 1, 4),
    "self3000_K1": lambda: _self(3000, 2, 1),
    "self3000_K4": lambda: _self(3000, 2, 4),
    "self3000_K8": lambda: _self(3000, 2, 8),
    "self3000_K16": lambda: _self(3000, 2, 16),
    "outside_257x1000": _outside,
    "twice200": _twice,
    "flat1500": _flat,
    "pad_P2_3_K4": lambda: dict(p1=_uniform(70, 61)[None], p2=_uniform(3, 62)[None], K=4),
    "one_query": lambda: dict(p1=_uniform(1, 71)[None], p2=_uniform(500, 72)[None], K=4),
    "batch2": _batch2,
}
CASES = tuple(BUILDERS)
_CASES, _ORACLES, _HOST = {}, {}, []


def case(name):
    if name not in _CASES:
        c = BUILDERS[name]()
        c = {k: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for k, v in c.items()}
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CASES[name] = c
    return _CASES[name]


def dist64(q, pts):
    """(P1,3), (P2,3) float32 -> (P1,P2) float64 squared distances"""
    d = q.astype(np.float64)[:, None, :] - pts.astype(np.float64)[None, :, :]
    return (d * d).sum(-1)


def oracle(name):
    """-> dict(idx (N,P1,K) int64, dists (N,P1,K) float64, kth (N,P1) the K-th distance (inf where P2 < K), marginal (N,P1) bool):
    computed once per case and left unchanged."""
    if name in _ORACLES:
        return _ORACLES[name]
    c = case(name)
    p1, p2, K = c["p1"], c["p2"], c["K"]
    N, P1, P2 = p1.shape[0], p1.shape[1], p2.shape[1]
    idx = np.zeros((N, P1, K), np.int64)
    dists = np.zeros((N, P1, K), np.float64)
    kth = np.full((N, P1), np.inf)
    marginal = np.zeros((N, P1), bool)
    for n in range(N):
        for a in range(0, P1, 512):
            d = dist64(p1[n, a:a + 512], p2[n])
            order = np.argsort(d, axis=1, kind="stable")[:, :K + 1]
            near = np.take_along_axis(d, order, axis=1)
            m = min(K, P2)
            idx[n, a:a + 512, :m], dists[n, a:a + 512, :m] = order[:, :m], near[:, :m]
            if P2 >= K:
                kth[n, a:a + 512] = near[:, K - 1]
            lo, hi = near[:, :-1], near[:, 1:]
            same = (p2[n][order[:, :-1]] == p2[n][order[:, 1:]]).all(-1)
            marginal[n, a:a + 512] = (((hi - lo) < GAP * hi) & ~same).any(1)
    out = dict(idx=idx, dists=dists, kth=kth, marginal=marginal)
    for v in out.values():
        v.setflags(write=False)
    _ORACLES[name] = out
    return out


def check(name, dists, idx):
    """Holds idx, the padding and the order of a result (numpy, (N,P1,K)) to the oracle -> (marginal rows, the largest error of
    dists in units of its bar DIST_REL d + DIST_ABS: the caller prints it, then asserts that it is <= 1)"""
    c, ref = case(name), oracle(name)
    p1, p2, K = c["p1"], c["p2"], c["K"]
    N, P1, P2 = p1.shape[0], p1.shape[1], p2.shape[1]
    assert dists.shape == (N, P1, K) and idx.shape == (N, P1, K) and dists.dtype == np.float32 and idx.dtype == np.int64
    assert (idx >= 0).all() and (idx < max(P2, 1)).all()
    firm = ~ref["marginal"]
    assert np.array_equal(idx[firm], ref["idx"][firm]), f"{name}: idx differs from the oracle on a row that is not marginal"
    m = min(K, P2)
    assert (idx[..., m:] == 0).all() and (dists[..., m:] == 0).all(), f"{name}: the padding is not (0, 0)"
    worst = 0.0
    for n in range(N):
        true = ((p1[n].astype(np.float64)[:, None, :] - p2[n].astype(np.float64)[idx[n, :, :m]]) ** 2).sum(-1)      # (P1, m)
        assert (true <= ref["kth"][n][:, None] * (1 + GAP)).all(), f"{name}: a chosen neighbour lies beyond the K-th distance"
        err = np.abs(dists[n, :, :m].astype(np.float64) - true)
        bar = DIST_REL * true + DIST_ABS
        worst = max(worst, float((err / bar).max()) if err.size else 0.0)
        assert (np.diff(dists[n, :, :m].astype(np.float64), axis=1) >= 0).all(), f"{name}: dists are not ascending"
    return int(ref["marginal"].sum()), worst


# ---- the g++ build ---------------------------------------------------------------------------------------------------------
def host_lib():
    """tests/hostcheck/knncheck.cpp as a shared library (g++ -ffp-contract=off, as the device build), once per process."""
    if not _HOST:
        src = os.path.join(ROOT, "tests", "hostcheck", "knncheck.cpp")
        out_dir = os.path.join(ROOT, "tests", "hostcheck", "_build")
        os.makedirs(out_dir, exist_ok=True)
        so = os.path.join(out_dir, "libknncheck.so")
        deps = [src, os.path.join(ROOT, "include", "d3ga.h")] + [os.path.join(ROOT, "d3ga_amd", "csrc", h) for h in ("knn_math.h", "mesh_raster_math.h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", so])
        _HOST.append(ctypes.CDLL(so))
    return _HOST[0]


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_knn(name, method="exhaustive"):
    """The g++ build's result of a case -> (dists (N,P1,K) float32, idx (N,P1,K) int64)"""
    c = case(name)
    return host_knn_arrays(c["p1"], c["p2"], c["K"], method)


def host_knn_arrays(p1, p2, K, method="exhaustive"):
    """The g++ build on p1 (N,P1,3), p2 (N,P2,3) float32.  method="grid" buckets p2 exactly as d3ga_amd.knn does (its `_grid`, on
    CPU tensors) and runs the ring search of knn_math.h."""
    import torch
    p1, p2 = np.ascontiguousarray(p1, np.float32), np.ascontiguousarray(p2, np.float32)
    N, P1, P2 = p1.shape[0], p1.shape[1], p2.shape[1]
    dists, idx = np.full((N, P1, K), np.nan, np.float32), np.full((N, P1, K), -7, np.int64)
    lib = host_lib()
    if method == "exhaustive":
        assert lib.hc_knn_points(N, P1, P2, K, _ptr(p1), _ptr(p2), _ptr(dists), _ptr(idx)) == 0
        return dists, idx
    from d3ga_amd.knn import _grid
    for n in range(N):
        start, items, origin_h, dims = _grid(torch.from_numpy(p2[n].copy()))
        start, items = np.ascontiguousarray(start.numpy()), np.ascontiguousarray(items.numpy())
        d, i = np.ascontiguousarray(dists[n]), np.ascontiguousarray(idx[n])
        q = np.ascontiguousarray(p1[n])
        assert lib.hc_knn_points_grid(P1, P2, K, _ptr(q), _ptr(np.ascontiguousarray(p2[n])), _ptr(start), _ptr(items), origin_h, dims,
                                      _ptr(d), _ptr(i)) == 0
        dists[n], idx[n] = d, i
    return dists, idx


def host_interp(pix_to_face, bary, attrs):
    """The g++ evaluation of d3ga_interp_face_attrs: pix_to_face (...,) int64, bary (...,3) float32, attrs (F,3,D) float32 -> (...,D)"""
    p2f, bary, attrs = (np.ascontiguousarray(pix_to_face, np.int64), np.ascontiguousarray(bary, np.float32), np.ascontiguousarray(attrs, np.float32))
    D = attrs.shape[2]
    out = np.full(p2f.shape + (D,), np.nan, np.float32)
    fn = host_lib().hc_interp_face_attrs
    fn.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int] + [ctypes.c_void_p] * 4
    assert fn(p2f.size, attrs.shape[0], D, _ptr(p2f), _ptr(bary), _ptr(attrs), _ptr(out)) == 0
    return out
