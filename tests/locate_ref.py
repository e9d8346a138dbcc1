"""The float64 oracles of the init-time point location (`tetra.compute_bary`) and 3-NN scale seed (`tetra.knn_mean_dist2`), the
inputs of their tests, and the g++ build of csrc/bary_math.h (tests/hostcheck/locatecheck.cpp) both test modules run.

compute_bary.  The oracle is oracle/bary.py (the reference's tetrahedron.h in float64, "largest minimum weight, then the lowest
index") with its margin report: m1 the winner's minimum weight, m2 the best among the other tets.
  * EXACT cases (cages and queries on dyadic lattices): every product of bary_math.h is exact in float32, so tetra_id, barys
    and active equal the oracle's bit for bit -- no tolerance, no marginal points, exact ties and `active` at exactly 0 included.
  * Otherwise a point is MARGINAL when m1 - m2 < EPS (which tet wins) or |m1| < EPS (whether it is active).  Away from the
    marginal points tetra_id and active are exactly the oracle's.  On them the chosen tet's float64 minimum weight is at least
    m1 - EPS, and active agrees with that tet's float64 minimum weight to EPS.  Everywhere barys stay within BARS["bary"] of the
    float64 weights of the tet chosen.
  * Marginal points are at most MARGINAL_CAP of the queries of a case that were not PLACED on a face: a query constructed as
    a face centroid of a conforming cage is marginal by construction (both neighbours hold it with minimum weight ~0) and is
    there to exercise the marginal rule; such queries are named by the case (`on_face`) and left out of the share.

knn_mean_dist2.  A float64 brute force over the float32 coordinates; the result stays within KNN_REL of it: 4 * 2^-24 per
squared distance (the budget tests/knn_ref.py derives for dx*dx + dy*dy + dz*dz) plus one rounding each for the sum and the
division by three.  On the EXACT clouds (dyadic lattices) it is the float32 value of ((d0 + d1) + d2) / 3.0f.
"""
import ctypes
import os
import subprocess

import numpy as np

from conftest import ROOT

EPS = 1e-5
MARGINAL_CAP = 0.02
KNN_REL, KNN_ABS = 6 * 2.0 ** -24, 2.0 ** -149

# Value bar of barys: 8 x the largest |w_host - w_float64| of the g++ build over ALL cases that are not exact, rounded up to
# two digits (tests/test_locate_host.py::test_host_build_equals_the_oracle prints the measured value and holds the host build
# to bar / 8).  Weights are dimensionless; the cages' cells are about 0.15 .. 0.45 wide.
MEASURED = {"bary": 4.0e-6}
BARS = {k: 8 * v for k, v in MEASURED.items()}
# share of marginal queries per case, as printed by the same test (of the queries not placed on a face; in brackets of all)
MARGINAL_SHARES = {"jitter_T1": (0.0, 0.0977), "jitter_far": (0.0, 0.0337), "holes": (0.0, 0.05), "nonfinite": (0.0, 0.0977),
                   "flat_members": (0.0, 0.0977)}


# ---- cages ----------------------------------------------------------------------------------------------------------------
def _kuhn(n, lo, hi, jitter=0.0, seed=0):
    from d3ga_amd.synthetic import kuhn_cage
    verts, tets = kuhn_cage(n, np.asarray(lo, np.float64), np.asarray(hi, np.float64), jitter, np.random.default_rng(seed))
    return np.ascontiguousarray(verts[tets.astype(np.int64)], np.float32)            # (T,4,3)


def _lattice_points(n, lo, hi):
    """the half-cell lattice of an n-cell cage box from one half cell below to one above: (2 n + 3)^3 points"""
    step = (np.asarray(hi, np.float64) - np.asarray(lo, np.float64)) / (2 * n)
    k = np.arange(-1, 2 * n + 2)
    g = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3)
    return (np.asarray(lo, np.float64) + g * step).astype(np.float32)


def _dyadic4():
    pts = _lattice_points(8, 0.0, 1.0)                       # multiples of 1/16 in [-1/16, 17/16]: 19^3 = 6859
    return dict(points=pts, corners=_kuhn(4, 0.0, 1.0), exact=True)


def _dyadic4_perm():
    c = _dyadic4()
    order = np.random.default_rng(401).permutation(c["corners"].shape[0])
    return dict(points=c["points"], corners=np.ascontiguousarray(c["corners"][order]), exact=True)


FAR = np.array([1024.0, -512.0, 2048.0], np.float32)


def _dyadic4_far():
    c = _dyadic4()
    return dict(points=c["points"] + FAR, corners=c["corners"] + FAR, exact=True, same_as="dyadic4")


def _dyadic8_aniso():
    hi = np.array([1.0, 2.0, 0.5])
    step = hi / 16
    k = np.arange(-1, 18)
    g = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3)
    pts = (g * step).astype(np.float32) + np.float32(4096.0)
    return dict(points=pts, corners=_kuhn(8, 0.0, hi) + np.float32(4096.0), exact=True)


def _dyadic2():
    return dict(points=_lattice_points(4, 0.0, 1.0), corners=_kuhn(2, 0.0, 1.0), exact=True)


ONE_EACH = (1, 63, 64, 255, 256, 257, 513)


def _one_each(T):
    """T disjoint unit right tets, origins 2 apart on an 8 x 8 x . lattice; one query per tet at its centroid, in a seeded order"""
    t = np.arange(T)
    origin = np.stack([2 * (t % 8), 2 * ((t // 8) % 8), 2 * (t // 64)], -1).astype(np.float32)
    unit = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    corners = origin[:, None, :] + unit[None]
    order = np.random.default_rng(500 + T).permutation(T)
    pts = origin[order] + np.float32(0.25)
    return dict(points=pts, corners=corners, exact=True, expect_tid=order.astype(np.int64), expect_w=0.25)


P_EDGES = (1, 255, 256, 257, 513)


def _p_edge(P):
    c = _dyadic4()
    return dict(points=np.ascontiguousarray(c["points"][:P]), corners=c["corners"], exact=True)


def _twice():
    c = _dyadic4()
    return dict(points=c["points"], corners=np.concatenate([c["corners"], c["corners"]]), exact=True, same_as="dyadic4")


def _t1_boxes():
    from d3ga_amd.synthetic import _cage_boxes
    return _cage_boxes(2)


def _jitter_cage(boxes, seed):
    return np.concatenate([_kuhn(4, lo, hi, 0.2, seed + b) for b, (lo, hi) in enumerate(boxes)])


def _queries(corners, seed, n_in=2400, n_face=300, n_box=300):
    """inside by random barycentrics, face centroids, uniform in a box 1.3 x the cage -> (points, on_face)"""
    rng = np.random.default_rng(seed)
    T = corners.shape[0]
    w = rng.uniform(0.05, 1.0, (n_in, 4))
    w /= w.sum(1, keepdims=True)
    inside = (corners[rng.integers(0, T, n_in)].astype(np.float64) * w[:, :, None]).sum(1)
    faces = np.array([[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]])
    tri = corners[rng.integers(0, T, n_face)][np.arange(n_face)[:, None], faces[rng.integers(0, 4, n_face)]]
    face = tri.astype(np.float64).mean(1)
    lo, hi = corners.reshape(-1, 3).min(0).astype(np.float64), corners.reshape(-1, 3).max(0).astype(np.float64)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    box = rng.uniform(mid - 1.3 * half, mid + 1.3 * half, (n_box, 3))
    on_face = np.zeros(n_in + n_face + n_box, bool)
    on_face[n_in:n_in + n_face] = True
    return np.concatenate([inside, face, box]).astype(np.float32), on_face


def _jitter_t1():
    corners = _jitter_cage(_t1_boxes(), 610)
    pts, on_face = _queries(corners, 611)
    return dict(points=pts, corners=corners, exact=False, on_face=on_face)


def _jitter_far():
    c = _jitter_t1()
    return dict(points=c["points"] + np.float32(100.0), corners=c["corners"] + np.float32(100.0), exact=False, on_face=c["on_face"])


def _holes():
    """two jittered cages 0.5 apart along x; queries inside both, in the gap, and beyond the grid box on all six sides"""
    lo, hi = np.array([-0.3, -0.45, -0.2]), np.array([0.3, 0.45, 0.2])
    shift = np.array([1.1, 0.0, 0.0])
    corners = np.concatenate([_kuhn(4, lo, hi, 0.2, 620), _kuhn(4, lo + shift, hi + shift, 0.2, 621)])
    rng = np.random.default_rng(622)
    inside, on_face = _queries(corners, 623, 600, 60, 0)
    gap = rng.uniform([0.33, -0.45, -0.2], [0.77, 0.45, 0.2], (300, 3))
    glo, ghi = corners.reshape(-1, 3).min(0).astype(np.float64), corners.reshape(-1, 3).max(0).astype(np.float64)
    beyond = []
    for axis in range(3):
        for sign in (-1, 1):
            q = rng.uniform(glo, ghi, (40, 3))
            q[:, axis] = (ghi[axis] + rng.uniform(0.01, 3.0, 40)) if sign > 0 else (glo[axis] - rng.uniform(0.01, 3.0, 40))
            beyond.append(q)
    pts = np.concatenate([inside.astype(np.float64), gap] + beyond).astype(np.float32)
    return dict(points=pts, corners=corners, exact=False, on_face=np.concatenate([on_face, np.zeros(len(pts) - len(on_face), bool)]))


NONFINITE_ROWS = {7: (np.nan, None, None), 300: (None, np.inf, None), 1500: (None, None, -np.inf), 2500: (np.nan, np.nan, np.nan),
                  2999: (np.inf, -np.inf, np.inf)}


def _nonfinite():
    c = _jitter_t1()
    pts = c["points"].copy()
    for row, vals in NONFINITE_ROWS.items():
        for a, v in enumerate(vals):
            if v is not None:
                pts[row, a] = v
    return dict(points=pts, corners=c["corners"], exact=False, same_as="jitter_T1", on_face=c["on_face"],
                bad_rows=np.array(sorted(NONFINITE_ROWS)))


def vol6_f32(corners):
    """stp(b - a, c - a, d - a) of bary_math.h in numpy float32 (no contraction): what tet_weights divides by"""
    c = np.asarray(corners, np.float32)
    u, v, w = c[:, 1] - c[:, 0], c[:, 2] - c[:, 0], c[:, 3] - c[:, 0]
    return (u[:, 0] * (v[:, 1] * w[:, 2] - v[:, 2] * w[:, 1]) + u[:, 1] * (v[:, 2] * w[:, 0] - v[:, 0] * w[:, 2])
            + u[:, 2] * (v[:, 0] * w[:, 1] - v[:, 1] * w[:, 0]))


def flat_tets(points, seed, n_planar=24, n_repeat=8):
    """n_planar tets of four coplanar corners on tilted planes through query points -- candidates are drawn until enough have a
    float32 volume of exactly 0, which is what makes a tet degenerate for bary_math.h; the rest are slivers, out of scope -- and
    n_repeat tets with a repeated vertex (volume 0 whatever the other corners are)."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n_planar:
        q = points[rng.integers(0, len(points), 256)].astype(np.float64)
        u, v = rng.normal(size=(256, 3)), rng.normal(size=(256, 3))
        coef = rng.uniform(-0.3, 0.3, (256, 4, 2))
        coef[:, :, 0] -= coef[:, :, 0].mean(1, keepdims=True)              # the query is the corners' mean: inside the flat tet
        coef[:, :, 1] -= coef[:, :, 1].mean(1, keepdims=True)
        cand = (q[:, None, :] + coef[:, :, :1] * u[:, None, :] + coef[:, :, 1:] * v[:, None, :]).astype(np.float32)
        out.extend(cand[vol6_f32(cand) == 0.0][:n_planar - len(out)])
    rep = points[rng.integers(0, len(points), (n_repeat, 4))].copy()
    for k in range(n_repeat):                                 # corner 1, 2 or 3 repeats corner 0: an edge vector of exactly 0
        rep[k, 1 + k % 3] = rep[k, 0]
    flat = np.concatenate([np.stack(out), rep]).astype(np.float32)
    assert (vol6_f32(flat) == 0.0).all()
    return flat


def _flat_members():
    c = _jitter_t1()
    flat = flat_tets(c["points"], 640)
    return dict(points=c["points"], corners=np.concatenate([c["corners"], flat]), exact=False, same_as="jitter_T1", on_face=c["on_face"])


BUILDERS = {"dyadic4": _dyadic4, "dyadic4_perm": _dyadic4_perm, "dyadic4_far": _dyadic4_far, "dyadic8_aniso": _dyadic8_aniso,
            "dyadic2": _dyadic2, "twice": _twice, "jitter_T1": _jitter_t1, "jitter_far": _jitter_far, "holes": _holes,
            "nonfinite": _nonfinite, "flat_members": _flat_members}
BUILDERS.update({f"one_each_{T}": (lambda T=T: _one_each(T)) for T in ONE_EACH})
BUILDERS.update({f"P_edges_{P}": (lambda P=P: _p_edge(P)) for P in P_EDGES})
CASES = tuple(BUILDERS)
INEXACT = ("jitter_T1", "jitter_far", "holes")             # the cases with an oracle of their own and a margin protocol
_CASES, _ORACLES, _HOST, _HOSTRES = {}, {}, [], {}


def _freeze(c):
    c = {k: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def case(name):
    if name not in _CASES:
        _CASES[name] = _freeze(BUILDERS[name]())
    return _CASES[name]


def oracle(name):
    """-> dict(barys (P,4) f64, tid (P,) i64, active (P,) bool, m1, m2 (P,) f64, marginal (P,) bool): computed once per case and
    left unchanged.  A case that must reproduce another's results (`same_as`) has that case's oracle."""
    c = case(name)
    name = c.get("same_as", name)
    if name not in _ORACLES:
        from oracle import bary as ob
        c = case(name)
        b, t, a, m1, m2 = ob.compute_bary(c["points"], c["corners"], margins=True)
        out = dict(barys=b, tid=t, active=a, m1=m1, m2=m2, marginal=((m1 - m2) < EPS) | (np.abs(m1) < EPS))
        for v in out.values():
            v.setflags(write=False)
        _ORACLES[name] = out
    return _ORACLES[name]


def marginal_share(name):
    """-> (share among the queries not placed on a face, share among all)"""
    c, ref = case(name), oracle(name)
    free = ~c["on_face"] if "on_face" in c else np.ones(len(ref["marginal"]), bool)
    return float(ref["marginal"][free].mean()), float(ref["marginal"].mean())


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def check_bary(name, barys, tid, active):
    """Holds a result (numpy: barys (P,4) float32, tid (P,) int64, active (P,) bool) to the oracle of the case.  -> the largest
    |barys - float64 weights of the chosen tet| (0 on an exact case): the caller prints it, then asserts it against its bar."""
    from oracle import bary as ob
    c, ref = case(name), oracle(name)
    P, T = c["points"].shape[0], c["corners"].shape[0]
    assert barys.shape == (P, 4) and barys.dtype == np.float32 and tid.shape == (P,) and tid.dtype == np.int64
    assert active.shape == (P,) and active.dtype == np.bool_
    assert (tid >= 0).all() and (tid < T).all()
    good = np.ones(P, bool)
    if "bad_rows" in c:                                       # a coordinate that is not finite: (0, 0, False), no other row moves
        bad = c["bad_rows"]
        good[bad] = False
        assert (bits(barys[bad]) == 0).all() and (tid[bad] == 0).all() and not active[bad].any(), f"{name}: a row that is not finite"
    if "expect_tid" in c:
        assert np.array_equal(tid, c["expect_tid"]), f"{name}: tetra_id is not the inverse permutation"
        assert (barys == np.float32(c["expect_w"])).all() and active.all(), name
    if name == "twice":
        assert (tid < T // 2).all(), "twice: the second copy of a tet was chosen"
    if c["exact"]:
        assert np.array_equal(tid, ref["tid"]), f"{name}: tetra_id differs from the oracle ({int((tid != ref['tid']).sum())} rows)"
        assert np.array_equal(barys.astype(np.float64), ref["barys"]), f"{name}: barys differ from the oracle"
        assert np.array_equal(active, ref["active"]), f"{name}: active differs from the oracle"
        return 0.0
    firm = good & ~ref["marginal"]
    assert np.array_equal(tid[firm], ref["tid"][firm]), f"{name}: tetra_id differs from the oracle on {int((tid[firm] != ref['tid'][firm]).sum())} rows that are not marginal"
    assert np.array_equal(active[firm], ref["active"][firm]), f"{name}: active differs from the oracle on a row that is not marginal"
    if name in ("nonfinite", "flat_members"):                 # the tets of jitter_T1 are the first of the case
        corners = case("jitter_T1")["corners"]
        assert (tid < corners.shape[0]).all(), f"{name}: a zero-volume tet was chosen"
    else:
        corners = c["corners"]
    w64, mn64 = ob.min_weight(c["points"][good], corners, tid[good])
    soft = ref["marginal"][good]
    assert (mn64[soft] >= ref["m1"][good][soft] - EPS).all(), f"{name}: a marginal point sits in a tet that is not among the best"
    act = active[good]
    assert (mn64[act] >= -EPS).all() and (mn64[~act] < EPS).all(), f"{name}: active contradicts the chosen tet's minimum weight"
    return float(np.abs(barys[good].astype(np.float64) - w64).max())


# ---- 3-NN clouds -----------------------------------------------------------------------------------------------------------
def _grid_cloud(nx, ny, nz, scale, offset=0.0):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    return (g.astype(np.float32) * np.float32(scale) + np.float32(offset)).astype(np.float32)


def _uniform(P, seed, lo=0.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, (P, 3)).astype(np.float32)


def _outlier():
    p = _uniform(2500, 704, 0.0, 0.25)
    p[1234] = 64.0
    return p


KNN_BUILDERS = {
    "lattice16x16x8": (lambda: _grid_cloud(16, 16, 8, 0.25), True),                 # P = 2048 exactly
    "lattice13_far": (lambda: _grid_cloud(13, 13, 13, 0.125, 256.0), True),
    "planar47": (lambda: _grid_cloud(47, 47, 1, 0.0625), True),                     # grid dimensions 257 x 257 x 1
    "planar257x9": (lambda: _grid_cloud(257, 9, 1, 0.1), False),                    # h = 0.1: Python and the kernel bucket 333 points differently
    "line2100": (lambda: _grid_cloud(2100, 1, 1, 0.3), False),
    "duplicates": (lambda: (np.random.default_rng(703).integers(0, 16, (2500, 3)) / 64.0).astype(np.float32), True),
    "outlier": (_outlier, False),
    "translated": (lambda: _uniform(2500, 705) + np.float32(1000.0), False),
}
KNN_SMALL = (1, 2, 3, 4, 2047, 2049)
KNN_BUILDERS.update({f"uniform{P}": ((lambda P=P: _uniform(P, 710 + P)), False) for P in KNN_SMALL})
KNN_CASES = tuple(KNN_BUILDERS)
_KNN, _KNN_ORACLES, _KNN_HOST = {}, {}, {}


def knn_case(name):
    """-> (points (P,3) float32, exact)"""
    if name not in _KNN:
        p = np.ascontiguousarray(KNN_BUILDERS[name][0](), np.float32)
        p.setflags(write=False)
        _KNN[name] = (p, KNN_BUILDERS[name][1])
    return _KNN[name]


def knn3_f64(p):
    """float64 brute force: (P,3) float32 -> (P,3) the three smallest squared distances to OTHER points, ascending, inf where
    there is none"""
    P = p.shape[0]
    out = np.full((P, 3), np.inf)
    q = p.astype(np.float64)
    for a in range(0, P, 512):
        d = ((q[a:a + 512, None, :] - q[None, :, :]) ** 2).sum(-1)
        d[np.arange(d.shape[0]), np.arange(a, a + d.shape[0])] = np.inf
        k = min(3, P - 1)
        if k:
            out[a:a + 512, :k] = np.sort(np.partition(d, k - 1, axis=1)[:, :k], axis=1)
    return out


def knn_oracle(name):
    """-> dict(near (P,3) f64, mean (P,) f64 = sum of what exists / 3, exact32 (P,) float32 or None)"""
    if name not in _KNN_ORACLES:
        p, exact = knn_case(name)
        near = knn3_f64(p)
        have = np.where(np.isfinite(near), near, 0.0)
        exact32 = None
        if exact:
            d = have.astype(np.float32)
            assert np.array_equal(d.astype(np.float64), have), f"{name}: not an exact cloud"
            exact32 = ((d[:, 0] + d[:, 1]) + d[:, 2]) / np.float32(3.0)
            exact32.setflags(write=False)
        out = dict(near=near, mean=have.sum(1) / 3.0, exact32=exact32)
        out["near"].setflags(write=False)
        out["mean"].setflags(write=False)
        _KNN_ORACLES[name] = out
    return _KNN_ORACLES[name]


def check_knn(name, out):
    """Holds a result (numpy (P,) float32) to the oracle -> its largest error in units of the bar KNN_REL mean + KNN_ABS."""
    p, exact = knn_case(name)
    ref = knn_oracle(name)
    assert out.shape == (p.shape[0],) and out.dtype == np.float32
    if exact:
        assert np.array_equal(bits(out), bits(ref["exact32"])), f"{name}: not the float32 value of ((d0 + d1) + d2) / 3"
    if not out.size:
        return 0.0
    return float((np.abs(out.astype(np.float64) - ref["mean"]) / (KNN_REL * ref["mean"] + KNN_ABS)).max())


# ---- the g++ build ---------------------------------------------------------------------------------------------------------
HOSTCHECK_SRC = os.path.join(ROOT, "tests", "hostcheck", "locatecheck.cpp")


def host_lib():
    """tests/hostcheck/locatecheck.cpp as a shared library (g++ -ffp-contract=off, as the device build), once per process."""
    if not _HOST:
        out_dir = os.path.join(ROOT, "tests", "hostcheck", "_build")
        os.makedirs(out_dir, exist_ok=True)
        so = os.path.join(out_dir, "liblocatecheck.so")
        deps = [HOSTCHECK_SRC] + [os.path.join(ROOT, "d3ga_amd", "csrc", h) for h in ("bary_math.h", "d3ga_math.h", "knn_math.h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", HOSTCHECK_SRC, "-o", so])
        _HOST.append(ctypes.CDLL(so))
    return _HOST[0]


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def reverse_lists(start, items):
    """CSR (start (n+1,), items) with every list reversed"""
    cell = np.repeat(np.arange(len(start) - 1), np.diff(start))
    out = np.empty_like(items)
    out[start[cell] + start[cell + 1] - 1 - np.arange(len(cell))] = items[:len(cell)]
    return out


def host_compute_bary_arrays(points, corners, method="grid", lib=None):
    """The g++ build on points (P,3), corners (T,4,3) float32 by the routes of `tetra.compute_bary`: method="grid" builds the grid
    with tetra._tet_grid (on CPU tensors), runs the grid search and sends the rows no candidate contains through the exhaustive
    one; T < 64 or P == 0 take the exhaustive route.  method="grid_reversed" is the grid route with every cell's list in descending
    order: the entry point promises nothing about the order of a list, the rule "equal and the lower index" is what makes the
    result independent of it (tetra._grid_csr happens to list ascending).  -> (barys (P,4) float32, tid (P,) int64, active (P,) bool)"""
    import torch
    lib = lib or host_lib()
    pts, cor = np.ascontiguousarray(points, np.float32), np.ascontiguousarray(corners, np.float32)
    P, T = pts.shape[0], cor.shape[0]
    barys, tid, act = np.full((P, 4), np.nan, np.float32), np.full((P,), -7, np.int32), np.full((P,), 9, np.uint8)
    if method == "exhaustive" or P == 0 or T < 64:
        assert lib.hc_compute_bary(P, T, _ptr(pts), _ptr(cor), _ptr(barys), _ptr(tid), _ptr(act)) == 0
        return barys, tid.astype(np.int64), act.astype(bool)
    from d3ga_amd.tetra import _tet_grid
    start, items, origin_h, dims = _tet_grid(torch.from_numpy(cor.copy()))
    start, items = np.ascontiguousarray(start.numpy()), np.ascontiguousarray(items.numpy())
    if method == "grid_reversed":
        items = reverse_lists(start, items)
    minw = np.full((P,), np.nan, np.float32)
    assert lib.hc_compute_bary_grid(P, _ptr(pts), _ptr(cor), _ptr(start), _ptr(items), origin_h, dims, _ptr(barys), _ptr(tid), _ptr(minw)) == 0
    active = minw >= 0.0
    outside = np.nonzero(~active)[0]
    if outside.size:
        sub = np.ascontiguousarray(pts[outside])
        n = sub.shape[0]
        b2, t2, a2 = np.full((n, 4), np.nan, np.float32), np.full((n,), -7, np.int32), np.full((n,), 9, np.uint8)
        assert lib.hc_compute_bary(n, T, _ptr(sub), _ptr(cor), _ptr(b2), _ptr(t2), _ptr(a2)) == 0
        barys[outside], tid[outside], active[outside] = b2, t2, a2.astype(bool)
    return barys, tid.astype(np.int64), active


def host_compute_bary(name, method="grid"):
    """The g++ build's result of a case, computed once per (case, method) and left unchanged."""
    if (name, method) not in _HOSTRES:
        c = case(name)
        res = host_compute_bary_arrays(c["points"], c["corners"], method)
        for v in res:
            v.setflags(write=False)
        _HOSTRES[(name, method)] = res
    return _HOSTRES[(name, method)]


def host_knn_arrays(points, method="exhaustive", lib=None):
    """The g++ build of the 3-NN mean on (P,3) float32.  method="grid" buckets the points with tetra._point_grid (on CPU tensors)
    and runs the ring search, whatever P >= 1 is (the device entry takes that route from 2048 points)."""
    import torch
    lib = lib or host_lib()
    pts = np.ascontiguousarray(points, np.float32)
    P = pts.shape[0]
    out = np.full((P,), np.nan, np.float32)
    if method == "exhaustive" or P == 0:
        assert lib.hc_knn3_mean_dist2(P, _ptr(pts), _ptr(out)) == 0
        return out
    from d3ga_amd.tetra import _point_grid
    start, items, origin_h, dims = _point_grid(torch.from_numpy(pts.copy()))
    start, items = np.ascontiguousarray(start.numpy()), np.ascontiguousarray(items.numpy())
    assert lib.hc_knn3_mean_dist2_grid(P, _ptr(pts), _ptr(start), _ptr(items), origin_h, dims, _ptr(out)) == 0
    return out


def host_knn(name, method="exhaustive"):
    if (name, method) not in _KNN_HOST:
        out = host_knn_arrays(knn_case(name)[0], method)
        out.setflags(write=False)
        _KNN_HOST[(name, method)] = out
    return _KNN_HOST[(name, method)]
