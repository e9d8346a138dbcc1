"""The oracle of quadric edge-collapse decimation (d3ga_amd/cage_author.py::decimate) in numpy, restated from the rules
and not from the header's code: every float64 step is an elementwise numpy operation in the order the rules state (no
`np.linalg.solve`, no `np.dot`), connectivity comes from the oracle's own plan (template_bind_ref.plan), Python sets and dicts.  A
last-bit difference in a cost can change which edge wins, so the comparison with the g++ build is equality of bits.

Below it the g++ build of csrc/decimate_math.h (tests/hostcheck/decimate_host.cpp), the text the kernels run, driven round by round
as the Python layer drives the kernels, and the shapes the tests share."""
import ctypes
import os
import subprocess

import numpy as np

import cage_author_ref as ca
import gauss_init_ref as gr
import template_bind_ref as tr

ROOT = tr.ROOT
STATUS_RANGE, STATUS_STUCK = 1, 8                            # D3GA_CAGE_STATUS_* (include/d3ga.h)
MAX_ROUNDS = 4096                                            # D3GA_CAGE_MAX_ITERATIONS
BAD_KEY = tr.BAD_KEY
FLT_MAX = 3.4028234663852886e38
_p = gr._p


# ---- the rules ------------------------------------------------------------------------------------------------------------------------
def _cross(d, e):
    return d[:, 1] * e[:, 2] - d[:, 2] * e[:, 1], d[:, 2] * e[:, 0] - d[:, 0] * e[:, 2], d[:, 0] * e[:, 1] - d[:, 1] * e[:, 0]


def quadrics(x, f):
    """rule 1 -> (V,10): per vertex the faces' area-weighted plane quadrics added in ascending face index"""
    V = len(x)
    a, b, c = x[f[:, 0]], x[f[:, 1]], x[f[:, 2]]
    nx, ny, nz = _cross(b - a, c - a)
    with np.errstate(all="ignore"):
        ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
        has = ln > 0
        area = ln / 2.0
        mx, my, mz = nx / ln, ny / ln, nz / ln
        p = [mx, my, mz, -((mx * a[:, 0] + my * a[:, 1]) + mz * a[:, 2])]
        K = np.stack([area * (p[i] * p[j]) for i in range(4) for j in range(i, 4)], 1)
    offsets, idx = ca.vertex_faces(f, V)
    deg = offsets[1:] - offsets[:-1]
    Q = np.zeros((V, 10))
    for j in range(int(deg.max()) if V else 0):              # the j-th face of every vertex that has one: ascending order
        who = np.nonzero(deg > j)[0]
        face = idx[offsets[who] + j]
        who, face = who[has[face]], face[has[face]]
        Q[who] = Q[who] + K[face]
    return Q


def cost(q, p):
    """rule 3d: (n,10), (n,3) -> the clamped cost, +inf where it is not finite"""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        t0 = ((q[:, 0] * x + q[:, 1] * y) + q[:, 2] * z) + q[:, 3]
        t1 = ((q[:, 1] * x + q[:, 4] * y) + q[:, 5] * z) + q[:, 6]
        t2 = ((q[:, 2] * x + q[:, 5] * y) + q[:, 7] * z) + q[:, 8]
        t3 = ((q[:, 3] * x + q[:, 6] * y) + q[:, 8] * z) + q[:, 9]
        c = ((x * t0 + y * t1) + z * t2) + t3
    return np.where(np.isfinite(c), np.where(c > 0, c, 0.0), np.inf)


def place(q, xu, xw):
    """rule 3d -> (points (n,3), costs (n,), solved (n,) bool)"""
    xx, xy, xz, yy, yz, zz = q[:, 0], q[:, 1], q[:, 2], q[:, 4], q[:, 5], q[:, 7]
    with np.errstate(all="ignore"):
        amax = np.abs(q[:, [0, 1, 2, 4, 5, 7]]).max(1)
        m00, m01, m02 = yy * zz - yz * yz, xy * zz - yz * xz, xy * yz - yy * xz
        det = (xx * m00 - xy * m01) + xz * m02
        solved = np.abs(det) > 1e-10 * ((amax * amax) * amax)
        i01, i11, i12, i22 = xz * yz - xy * zz, xx * zz - xz * xz, xy * xz - xx * yz, xx * yy - xy * xy
        r0, r1, r2 = -q[:, 3], -q[:, 6], -q[:, 8]
        best = np.stack([((m00 * r0 + i01 * r1) + m02 * r2) / det, ((i01 * r0 + i11 * r1) + i12 * r2) / det, ((m02 * r0 + i12 * r1) + i22 * r2) / det], 1)
    mid = (xu + xw) * 0.5
    point, c = xu.copy(), cost(q, xu)
    for other in (xw, mid):                                  # ties stay with the earlier one
        co = cost(q, other)
        better = co < c
        point[better], c[better] = other[better], co[better]
    point[solved] = best[solved]
    c = np.where(solved, cost(q, np.where(solved[:, None], best, 0.0)), c)
    return point, c, solved


def keys_of(costs, edges):
    bits = np.minimum(costs, FLT_MAX).astype(np.float32).view(np.uint32).astype(np.int64)
    return (bits << 32) | edges.astype(np.int64)


def candidates(p, x, Q, f):
    """rule 3 over the oracle's plan -> (keys (E,) int64 with BAD_KEY for an invalid edge, points (E,3))"""
    E, V = p["E"], p["V"]
    u, w = p["edge_verts"][:, 0].astype(np.int64), p["edge_verts"][:, 1].astype(np.int64)
    a, b = p["edge_opp"][:, 0].astype(np.int64), p["edge_opp"][:, 1].astype(np.int64)
    off, nbr = p["vert_offsets"], p["vert_nbr"]
    ring = [set(nbr[off[v]:off[v + 1]].tolist()) for v in range(V)]
    vb = p["vert_boundary"].astype(bool)
    valid = ~(vb[u] | vb[w] | p["edge_boundary"].astype(bool))                               # (a)
    edge_at = {(int(lo), int(hi)): e for e, (lo, hi) in enumerate(p["edge_verts"].tolist())}
    for e in np.nonzero(valid)[0]:
        if ring[u[e]] & ring[w[e]] != {int(a[e]), int(b[e])} or a[e] == b[e]:                # (b)
            valid[e] = False
            continue
        other = edge_at.get((int(min(a[e], b[e])), int(max(a[e], b[e]))))
        if other is not None and set(p["edge_opp"][other].tolist()) == {int(u[e]), int(w[e])}:          # (c)
            valid[e] = False
    point, c, _ = place(Q[u] + Q[w], x[u], x[w])                                              # (d)
    valid &= np.isfinite(c)
    offsets, idx = ca.vertex_faces(f, V)
    pair_edge, pair_face, pair_end = [], [], []
    for e in np.nonzero(valid)[0]:                                                            # (e)
        for end, other in ((u[e], w[e]), (w[e], u[e])):
            faces = idx[offsets[end]:offsets[end + 1]]
            faces = faces[(f[faces] != other).all(1)]
            pair_edge += [e] * len(faces)
            pair_face += faces.tolist()
            pair_end += [end] * len(faces)
    if pair_edge:
        pe, pf, pend = np.array(pair_edge), np.array(pair_face), np.array(pair_end)
        tri = f[pf]
        old = [x[tri[:, k]] for k in range(3)]
        new = [np.where((tri[:, k] == pend)[:, None], point[pe], old[k]) for k in range(3)]
        n = _cross(old[1] - old[0], old[2] - old[0])
        t = _cross(new[1] - new[0], new[2] - new[0])
        skipped = (n[0] == 0) & (n[1] == 0) & (n[2] == 0)
        with np.errstate(all="ignore"):
            flips = ~skipped & ~(((n[0] * t[0] + n[1] * t[1]) + n[2] * t[2]) > 0)
        valid[np.unique(pe[flips])] = False
    keys = np.where(valid, keys_of(np.where(valid, c, 0.0), np.arange(E)), BAD_KEY)
    return keys, point


def decimate(vertices, faces, target, max_rounds=MAX_ROUNDS):
    """-> (vertices float32, faces int32, rounds, status)"""
    x, f = np.array(vertices, np.float64), np.asarray(faces, np.int64).reshape(-1, 3).copy()
    V = len(x)
    rounds, status, Q = 0, 0, None
    while True:
        need = (len(f) - target + 1) // 2
        if need <= 0:
            break
        if rounds >= max_rounds:
            status |= STATUS_STUCK
            break
        p = tr.plan(f, V)
        tr.check_status(p["status"])
        if Q is None:
            Q = quadrics(x, f)
        keys, point = candidates(p, x, Q, f)
        rounds += 1
        admitted = np.sort(keys[keys != BAD_KEY])[:need]
        if len(admitted) == 0:
            status |= STATUS_STUCK
            break
        ends = p["edge_verts"][admitted & 0xffffffff].astype(np.int64)
        owner = np.full(V, np.iinfo(np.int64).max)
        np.minimum.at(owner, ends[:, 0], admitted)
        np.minimum.at(owner, ends[:, 1], admitted)
        off, nbr = p["vert_offsets"], p["vert_nbr"]
        remap = np.arange(V)
        moved = []
        for key, (u, w) in zip(admitted.tolist(), ends.tolist()):
            around = np.concatenate([[u, w], nbr[off[u]:off[u + 1]], nbr[off[w]:off[w + 1]]])
            if (owner[around] >= key).all():
                moved.append((u, w, key & 0xffffffff))
        for u, w, e in moved:                                # their closed neighbourhoods are disjoint: any order
            x[u] = point[e]
            Q[u] = Q[u] + Q[w]
            remap[w] = u
        f = remap[f]
        f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])]
    return finish(x, f) + (rounds, status)


def finish(x, f):
    """rule 7: the vertices no face names removed in ascending order, one rounding to float32"""
    used = np.zeros(len(x), bool)
    used[f.reshape(-1)] = True
    return x[used].astype(np.float32), (np.cumsum(used) - 1)[f].astype(np.int32)


# ---- first principles -----------------------------------------------------------------------------------------------------------------
def euler(faces):
    f = np.asarray(faces, np.int64)
    return len(np.unique(f)) - ca.edge_census(f)[2] + len(f)


def parts(faces):
    return len(np.unique(ca.components(faces)))


def surface_error(vertices, faces, fine_vertices, fine_faces):
    """-> (max, mean) distance from the vertices and face centroids of a mesh to the fine surface, |volume - fine volume|"""
    v, f = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)
    fv = np.asarray(fine_vertices, np.float64)
    points = np.concatenate([v, v[f].mean(1)])
    d = ca.point_triangle_distance(points, fv[np.asarray(fine_faces, np.int64)])
    return float(d.max()), float(d.mean()), abs(ca.signed_volume(v, f) - ca.signed_volume(fv, fine_faces))


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------
def icosphere(levels=3, seed=0, jitter=0.004, squash=(1.0, 0.8, 0.55)):
    """the icosahedron split `levels` times and pushed onto the unit sphere (F = 20 4^levels), squashed and jittered"""
    t = (1 + 5 ** 0.5) / 2
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    v = [list(map(float, r)) for r in v]
    for _ in range(levels):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                mid[key] = len(v)
                v.append([(v[a][i] + v[b][i]) / 2 for i in range(3)])
            return mid[key]
        for a, b, c in f:
            ab, bc, ca_ = m(a, b), m(b, c), m(c, a)
            nf += [[a, ab, ca_], [ab, b, bc], [ca_, bc, c], [ab, bc, ca_]]
        f = nf
    v = np.array(v)
    v = v / np.linalg.norm(v, axis=1, keepdims=True) * np.array(squash)
    return v + np.random.default_rng([seed, levels, 23]).normal(0, jitter, v.shape), np.array(f, np.int32)


def octahedron():
    return tr.sphere(0)


def with_unreferenced(v, f):
    """the same mesh with a vertex no face names put in at row 3"""
    v2 = np.insert(v, 3, [9.0, 9.0, 9.0], axis=0)
    return v2, np.where(f >= 3, f + 1, f).astype(np.int32)


def host_cases():
    """(name, vertices float64, faces int32, target): the meshes the host test and the GPU test both run"""
    v, f = icosphere(3)
    yield "icosphere 1280 -> 128", v, f, 128
    v, f = ca.capsule_figure(r=8)
    yield "capsule figure r=8 -> 400", v, f, 400
    v, f = ca.mesh_of(ca.torus_grid(5), 5, 0.002)                # 1 440 faces
    yield "torus -> a quarter", v, f, len(f) // 4


def small_cases():
    """(name, vertices, faces, target, max_rounds): the edge cases"""
    yield ("tetrahedron -> 2",) + tr.tetrahedron() + (2, MAX_ROUNDS)
    yield ("octahedron -> 4",) + octahedron() + (4, MAX_ROUNDS)
    yield ("open 17 x 17 grid -> 300",) + tr.grid(17, 17, jitter=0.1) + (300, MAX_ROUNDS)
    yield ("open 17 x 17 grid -> 2",) + tr.grid(17, 17, jitter=0.1) + (2, MAX_ROUNDS)
    yield ("bipyramid over a 70-gon -> 40",) + tr.bipyramid(70) + (40, MAX_ROUNDS)
    yield ("an unreferenced vertex",) + with_unreferenced(*icosphere(1)) + (40, MAX_ROUNDS)
    yield ("one round only",) + icosphere(2) + (60, 1)
    yield ("target >= F",) + icosphere(1) + (80, MAX_ROUNDS)


# ---- the g++ build of csrc/decimate_math.h ----------------------------------------------------------------------------------------------
class DecimateStruct(ctypes.Structure):
    _fields_ = [("n_admit", ctypes.c_int32), ("reserved", ctypes.c_int32)] + \
               [(n, ctypes.c_void_p) for n in ("x", "quadrics", "faces", "csr_offsets", "csr_faces", "keys", "placement", "sorted_keys", "owner", "remap",
                                               "faces_out", "scratch")] + \
               [("scratch_bytes", ctypes.c_int64), ("counts", ctypes.c_void_p), ("status", ctypes.c_void_p)]


STAGES = ("hc_decimate_quadrics", "hc_decimate_candidates", "hc_decimate_collapse", "hc_decimate_faces")
_LIB = []


def lib():
    if not _LIB:
        src = os.path.join(ROOT, "tests", "hostcheck", "decimate_host.cpp")
        out_dir = os.path.join(ROOT, "tests", "hostcheck", "_build")
        os.makedirs(out_dir, exist_ok=True)
        so = os.path.join(out_dir, "libdecimate_host.so")
        deps = [src, os.path.join(ROOT, "include", "d3ga.h")] + [os.path.join(ROOT, "d3ga_amd", "csrc", h)
                                                                 for h in ("decimate_math.h", "cage_author_math.h", "gauss_init_math.h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", so])
        L = ctypes.CDLL(so)
        L.hc_decimate_scratch_bytes.argtypes, L.hc_decimate_scratch_bytes.restype = [ctypes.c_int32], ctypes.c_int64
        for name in STAGES:
            getattr(L, name).argtypes = [ctypes.POINTER(tr.PlanStruct), ctypes.POINTER(DecimateStruct)]
        _LIB.append(L)
    return _LIB[0]


def host_decimate(vertices, faces, target, max_rounds=MAX_ROUNDS):
    """The g++ build, round by round as `d3ga_amd.decimate` drives the kernels -> (vertices float32, faces int32, rounds, status).
    The sort between candidates and collapse is numpy's."""
    L = lib()
    x, f = np.array(vertices, np.float64, order="C"), np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    V = len(x)
    Q, owner, remap = np.full((V, 10), np.nan), np.full(V, 7, np.uint64), np.full(V, -7, np.int32)
    counts, status = np.full(2, -7, np.int64), np.zeros(1, np.uint32)
    nbytes = L.hc_decimate_scratch_bytes(len(f))
    scratch = gr._aligned(nbytes)
    scratch[:] = 0xEE                                        # the scratch needs no initialisation
    d = DecimateStruct(x=x.ctypes.data, quadrics=Q.ctypes.data, owner=owner.ctypes.data, remap=remap.ctypes.data, scratch=scratch.ctypes.data,
                       scratch_bytes=nbytes, counts=counts.ctypes.data, status=status.ctypes.data)
    rounds = 0
    while True:
        need = (len(f) - target + 1) // 2
        if need <= 0:
            break
        if rounds >= max_rounds:
            status[0] |= STATUS_STUCK
            break
        p = tr.host_plan(f, V)
        tr.check_status(p["status"])
        st = tr._struct(p)
        offsets, idx = ca.vertex_faces(f, V)
        keys, placement, f_next = np.full(p["E"], -7, np.int64), np.full((p["E"], 3), np.nan), np.full_like(f, -7)
        d.faces, d.csr_offsets, d.csr_faces, d.keys, d.placement, d.faces_out = (a.ctypes.data for a in (f, offsets, idx, keys, placement, f_next))
        if rounds == 0:
            assert L.hc_decimate_quadrics(ctypes.byref(st), ctypes.byref(d)) == 0
        assert L.hc_decimate_candidates(ctypes.byref(st), ctypes.byref(d)) == 0
        sorted_keys = np.sort(keys)
        d.sorted_keys, d.n_admit = sorted_keys.ctypes.data, min(need, p["E"])
        assert L.hc_decimate_collapse(ctypes.byref(st), ctypes.byref(d)) == 0
        assert L.hc_decimate_faces(ctypes.byref(st), ctypes.byref(d)) == 0
        rounds += 1
        if counts[1] == 0:
            status[0] |= STATUS_STUCK
            break
        f = np.ascontiguousarray(f_next[:counts[0]])
    return finish(x, f.astype(np.int64)) + (rounds, int(status[0]))


def host_tail(smoothed, faces, target):
    """what `simplify(..., decimation="quadric")` does after the Taubin filter, through the g++ builds -> (vertices float32, faces int32)"""
    v, f, _, st = host_decimate(smoothed, faces, target)
    assert st == 0
    return ca.keep_components(v, f, 70, True, ca.host_components(f, len(v)))


def large_cases():
    """(name, vertices, faces, target): the meshes only the GPU test runs (the g++ build is their reference)"""
    v, f = ca.capsule_figure(r=16, through_host_build=True)
    yield "capsule figure r=16 -> 1232", v, f, 1232            # 5 668 faces: 23 scan blocks, V and E no multiples of 256
    for name, r in (("ball r=25 -> a tenth", None), ("ball that fills the r=25 grid -> a tenth", 24.9)):
        v, f = ca.host_isosurface(ca.ball(25, r))              # 37 632 faces; 70 000: above 65 536, the block totals take a second pass
        yield name, v.astype(np.float64) + np.random.default_rng(25).normal(0, 0.0005, v.shape), f, len(f) // 10


def same_result(a, b):
    """vertices, faces, rounds and status of two results equal bit for bit"""
    assert a[2:] == b[2:], (a[2:], b[2:])
    assert a[1].shape == b[1].shape and np.array_equal(a[1], b[1]), "faces"
    assert a[0].dtype == b[0].dtype == np.float32 and a[0].shape == b[0].shape and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), "vertices"
