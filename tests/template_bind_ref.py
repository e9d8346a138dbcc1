"""numpy oracle of template binding (d3ga_amd/template_bind.py, csrc/template_bind_math.h), written from the rules and
not from the kernels.  float64 numpy throughout, ONE rounding to float32 per output element, every sum in the order the rules state.

    edges     face edge h = 3 f + c joins (faces[f][c], faces[f][(c + 1) % 3]); unique edges ascending in (larger, smaller) endpoint; the
              members of an edge ascending in h: the first is the face of lower index, the second the other, a third is flagged and left
              out.  The opposite vertex of (f, c) is faces[f][(c + 2) % 3].  A face with an index outside [0, V) or a repeated vertex
              is flagged and takes no part.
    vertices  neighbours ascending; boundary vertex = an end of a boundary edge.
    odd       interior ((0.375 x0 + 0.375 x1) + x2 / 8) + x3 / 8; boundary (x0 + x1) 0.5.
    even      interior beta[k] S + (1 - k beta[k]) x; boundary S' / 8 + 0.75 x (S' over the neighbours that are boundary vertices); a
              vertex of no face keeps x.  S, S' start from 0 and add the neighbours in ascending order.
    faces     (a,o0,o2), (o0,b,o1), (o2,o1,c), (o0,o1,o2).
    nearest   float32 squared distances as csrc/knn_math.h states them, the lowest index on equal distances.
    unpose    [M t; 0 0 0 s] = the row's pairs in stored order, weight 0 skipped; x = adj(M) (v - t / s) / det - offset.

Below them the g++ build of csrc/template_bind_math.h (tests/hostcheck/template_bind_host.cpp), the text the kernels run, and the meshes
the tests share."""
import ctypes
import os
import subprocess

import numpy as np

import gauss_init_ref as gr

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
STATUS_RANGE, STATUS_NONMANIFOLD, STATUS_DEGENERATE, STATUS_SINGULAR = 1, 2, 4, 8       # D3GA_BIND_STATUS_* (include/d3ga.h)
BAD_KEY = 2 ** 63 - 1
MIN_DET = MIN_SCALE = 1e-12
PLAN_TABLES = ("edge_verts", "edge_opp", "edge_faces", "edge_boundary", "face_edge", "vert_offsets", "vert_nbr", "vert_boundary")
same_bits = gr.same_bits


def beta_table(max_valence):
    k = np.arange(1, int(max_valence) + 1, dtype=np.float64)
    out = np.zeros(int(max_valence) + 1, np.float64)
    out[1:] = (40.0 - (2.0 * np.cos(2 * np.pi / k) + 3) ** 2) / (64 * k)
    return out


# ---- topology ------------------------------------------------------------------------------------------------------------------------
def plan(faces, V):
    """-> dict of the plan's tables (PLAN_TABLES, numpy, the dtypes of the device tables) + V, F, E, max_valence, status"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    F = len(f)
    status = 0
    members = {}
    face_edge = np.full((F, 3), -1, np.int32)
    for i, t in enumerate(f.tolist()):
        if min(t) < 0 or max(t) >= V:
            status |= STATUS_RANGE
            continue
        if len(set(t)) < 3:
            status |= STATUS_DEGENERATE
            continue
        for c in range(3):
            a, b = t[c], t[(c + 1) % 3]
            members.setdefault((max(a, b), min(a, b)), []).append((i, c))
    order = sorted(members)                                  # ascending (larger, smaller)
    E = len(order)
    edge_verts, edge_opp = np.zeros((E, 2), np.int32), np.full((E, 2), -1, np.int32)
    edge_faces, edge_boundary = np.full((E, 2), -1, np.int32), np.zeros(E, np.uint8)
    nbrs = [[] for _ in range(V)]
    vert_boundary = np.zeros(V, np.uint8)
    for e, (hi, lo) in enumerate(order):
        ms = members[(hi, lo)]                               # ascending in (face, corner) by construction
        edge_verts[e] = lo, hi
        for slot, (i, c) in enumerate(ms[:2]):
            edge_faces[e, slot], edge_opp[e, slot] = i, f[i, (c + 2) % 3]
        for i, c in ms:
            face_edge[i, c] = e
        if len(ms) >= 3:
            status |= STATUS_NONMANIFOLD
        if len(ms) == 1:
            edge_boundary[e] = 1
            vert_boundary[lo] = vert_boundary[hi] = 1
        nbrs[lo].append(hi)
        nbrs[hi].append(lo)
    nbrs = [sorted(x) for x in nbrs]
    vert_offsets = np.zeros(V + 1, np.int32)
    vert_offsets[1:] = np.cumsum([len(x) for x in nbrs])
    vert_nbr = np.array([n for x in nbrs for n in x], np.int32).reshape(-1)
    return dict(V=V, F=F, E=E, max_valence=max([len(x) for x in nbrs] or [0]), status=status, edge_verts=edge_verts, edge_opp=edge_opp,
                edge_faces=edge_faces, edge_boundary=edge_boundary, face_edge=face_edge, vert_offsets=vert_offsets, vert_nbr=vert_nbr,
                vert_boundary=vert_boundary, faces=f)


# ---- stencils -------------------------------------------------------------------------------------------------------------------------
def stencil(p, x):
    """x (V, D) -> (V + E, D) float32 by the rules, over the oracle's plan p"""
    x = np.asarray(x, np.float64)
    V, E = p["V"], p["E"]
    D = x.shape[1]
    beta = beta_table(max(p["max_valence"], 1))
    off, nbr, vb = p["vert_offsets"].astype(np.int64), p["vert_nbr"], p["vert_boundary"].astype(bool)
    k = off[1:] - off[:-1]
    total, bound = np.zeros((V, D)), np.zeros((V, D))
    for j in range(int(k.max()) if V else 0):                # the j-th neighbour of every vertex that has one: ascending order
        has = np.nonzero(k > j)[0]
        n = nbr[off[has] + j]
        total[has] = total[has] + x[n]
        keep = vb[n]
        bound[has[keep]] = bound[has[keep]] + x[n[keep]]
    b = beta[k][:, None]
    interior = b * total + (1.0 - k[:, None].astype(np.float64) * b) * x
    even = np.where(vb[:, None], bound / 8.0 + 0.75 * x, interior)
    even = np.where((k == 0)[:, None], x, even)
    ev, eo = p["edge_verts"], p["edge_opp"]
    x0, x1 = x[ev[:, 0]], x[ev[:, 1]]
    is_b = p["edge_boundary"].astype(bool)
    x2, x3 = x[np.where(is_b, 0, eo[:, 0])], x[np.where(is_b, 0, eo[:, 1])]
    odd = np.where(is_b[:, None], (x0 + x1) * 0.5, ((0.375 * x0 + 0.375 * x1) + x2 / 8.0) + x3 / 8.0)
    return np.concatenate([even, odd]).astype(np.float32)


def new_faces(p):
    f, o = p["faces"], p["face_edge"].astype(np.int64) + p["V"]
    cols = [f[:, 0], o[:, 0], o[:, 2], o[:, 0], f[:, 1], o[:, 1], o[:, 2], o[:, 1], f[:, 2], o[:, 0], o[:, 1], o[:, 2]]
    return np.stack(cols, 1).reshape(-1, 3)


def check_status(status):
    if status & STATUS_RANGE:
        raise ValueError("an index outside its table")
    if status & STATUS_DEGENERATE:
        raise ValueError("a face names one vertex twice")
    if status & STATUS_NONMANIFOLD:
        raise ValueError("some edges are shared by more than 2 faces")
    if status & STATUS_SINGULAR:
        raise ValueError("a blended transform is singular")


def subdivide(vertices, faces, attrs=None, iterations=1):
    """-> (vertices' f32, faces' in the dtype of faces, attrs' f32 or None); raises ValueError as the Python layer does"""
    v, f = np.asarray(vertices), np.asarray(faces)
    a = None if attrs is None else np.asarray(attrs)
    dtype = f.dtype
    for _ in range(iterations):
        p = plan(f, len(v))
        check_status(p["status"])
        v = stencil(p, v)
        a = None if a is None else stencil(p, a) if a.shape[1] else np.zeros((len(v), 0), np.float32)
        f = new_faces(p)
    return v, f.astype(dtype), a


# ---- nearest vertex ---------------------------------------------------------------------------------------------------------------------
def _two_diff(a, b):
    c = -b
    s = a + c
    bp = s - a
    ap = s - bp
    return s, (a - ap) + (c - bp)


def knn_dist2(q, p):
    """(n,3), (m,3) float32 -> (n,m) float32: csrc/knn_math.h knn_dist2, operation by operation in float32"""
    q, p = np.asarray(q, np.float32), np.asarray(p, np.float32)
    with np.errstate(all="ignore"):
        d, e = zip(*[_two_diff(q[:, None, a], p[None, :, a]) for a in range(3)])
        plain = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        fixed = plain + np.float32(2) * ((d[0] * e[0] + d[1] * e[1]) + d[2] * e[2])
    return np.where(fixed == fixed, fixed, plain)


def nearest(template, query, chunk=512):
    """-> (n,) int64: the lowest index among the template vertices at the smallest float32 distance"""
    t, q = np.asarray(template, np.float32), np.asarray(query, np.float32)
    return np.concatenate([np.argmin(knn_dist2(q[a:a + chunk], t), axis=1) for a in range(0, len(q), chunk)]).astype(np.int64)


def nearest_margin(template, query, chunk=512):
    """float64: -> (best index, best squared distance, runner-up squared distance) per query"""
    t, q = np.asarray(template, np.float64), np.asarray(query, np.float64)
    idx, best, second = [], [], []
    for a in range(0, len(q), chunk):
        d = ((q[a:a + chunk, None, :] - t[None]) ** 2).sum(-1)
        i = np.argmin(d, axis=1)
        idx.append(i)
        best.append(d[np.arange(len(i)), i])
        d[np.arange(len(i)), i] = np.inf
        second.append(d.min(1) if t.shape[0] > 1 else np.full(len(i), np.inf))
    return np.concatenate(idx), np.concatenate(best), np.concatenate(second)


def inflate(vertices, faces, amount):
    v = np.asarray(vertices, np.float64)
    return v + amount * gr.vertex_normals_angle(v, faces) if amount else v


# ---- unpose ---------------------------------------------------------------------------------------------------------------------------
def unpose(vertices, joint_mats, skin, rows=None, offsets=None):
    """-> (x (n,3) float32, status).  skin: the dense table (R,J) or the pair (idx (R,K), w (R,K))"""
    v, A = np.asarray(vertices, np.float64), np.asarray(joint_mats, np.float64).reshape(-1, 16)
    n, J = len(v), len(A)
    if isinstance(skin, (tuple, list)):
        idx, w = np.asarray(skin[0], np.int64), np.asarray(skin[1], np.float64)
    else:
        w = np.asarray(skin, np.float64)
        idx = np.broadcast_to(np.arange(w.shape[1]), w.shape)
    R, K = w.shape
    r = np.arange(n) if rows is None else np.asarray(rows, np.int64)
    status = 0
    ok = (r >= 0) & (r < R)
    if offsets is not None:
        offsets = np.asarray(offsets, np.float64)
        ok &= r < len(offsets)
    rs = np.where(ok, r, 0)
    T, s = np.zeros((n, 12)), np.zeros(n)
    for k in range(K):
        wk, jk = w[rs, k], idx[rs, k]
        joint_ok = (jk >= 0) & (jk < J)
        use = ok & (wk != 0) & joint_ok
        if (ok & (wk != 0) & ~joint_ok).any():
            status |= STATUS_RANGE
        term = wk[:, None] * A[np.where(joint_ok, jk, 0), :12]
        T[use] = T[use] + term[use]
        s[use] = s[use] + wk[use]
    m = T.reshape(n, 3, 4)
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = (m[:, i, j] for i in range(3) for j in range(3))
    det = (m00 * (m11 * m22 - m12 * m21) - m01 * (m10 * m22 - m12 * m20)) + m02 * (m10 * m21 - m11 * m20)
    with np.errstate(all="ignore"):
        good = ok & (np.abs(det) >= MIN_DET) & (np.abs(s) >= MIN_SCALE) & np.isfinite(det) & np.isfinite(s)
        sd, dd = np.where(good, s, 1.0), np.where(good, det, 1.0)
        d0, d1, d2 = v[:, 0] - m[:, 0, 3] / sd, v[:, 1] - m[:, 1, 3] / sd, v[:, 2] - m[:, 2, 3] / sd
        c = [[m11 * m22 - m12 * m21, m02 * m21 - m01 * m22, m01 * m12 - m02 * m11],
             [m12 * m20 - m10 * m22, m00 * m22 - m02 * m20, m02 * m10 - m00 * m12],
             [m10 * m21 - m11 * m20, m01 * m20 - m00 * m21, m00 * m11 - m01 * m10]]
        x = np.stack([((c[i][0] * d0 + c[i][1] * d1) + c[i][2] * d2) / dd for i in range(3)], 1)
        if offsets is not None:
            x = x - offsets[np.where(ok, r, 0)]
        fits = (np.abs(x) <= 3.4028234663852886e38).all(1)
    if (~ok).any():
        status |= STATUS_RANGE
    if (ok & ~(good & fits)).any():
        status |= STATUS_SINGULAR
    return np.where((good & fits)[:, None], x, 0.0).astype(np.float32), status


def unpose_f64(vertices, joint_mats, skin, rows, offsets):
    """The same quantity with numpy's own float64 inverse of the 4x4 blend, unrounded: what a bound is taken against"""
    v, A = np.asarray(vertices, np.float64), np.asarray(joint_mats, np.float64).reshape(-1, 4, 4)
    T = np.einsum("vj,jab->vab", np.asarray(skin, np.float64), A)
    r = np.asarray(rows, np.int64)
    homo = np.concatenate([v, np.ones((len(v), 1))], 1)
    return np.einsum("vab,vb->va", np.linalg.inv(T)[r], homo)[:, :3] - np.asarray(offsets, np.float64)[r]


# ---- meshes ---------------------------------------------------------------------------------------------------------------------------
def tetrahedron():
    v = np.array([[1.0, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]])
    return v, np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)


def triangle():
    return np.array([[0.0, 0, 0], [1, 0, 0], [0.25, 1, 0.5]]), np.array([[0, 1, 2]], np.int32)


def quad():
    """two triangles over the diagonal 0-2: both of its ends have three boundary neighbours"""
    return np.array([[0.0, 0, 0], [1, 0, 0.25], [1.125, 0.875, 0], [0, 1, 0.5]]), np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def grid(nx, ny, seed=0, jitter=0.2):
    """an open nx x ny grid of vertices, two triangles per cell, alternating diagonals"""
    rng = np.random.default_rng([seed, nx, ny])
    xs, ys = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64), indexing="ij")
    v = np.stack([xs, ys, 0.3 * np.sin(xs) * np.cos(ys)], -1).reshape(-1, 3) + rng.uniform(-jitter, jitter, (nx * ny, 3))
    f = []
    for i in range(nx - 1):
        for j in range(ny - 1):
            a, b, c, d = i * ny + j, (i + 1) * ny + j, (i + 1) * ny + j + 1, i * ny + j + 1
            f += [[a, b, c], [a, c, d]] if (i + j) % 2 == 0 else [[a, b, d], [b, c, d]]
    return v, np.array(f, np.int32)


def torus(nx, ny, seed=0):
    """a closed nx x ny torus: every valence 6"""
    rng = np.random.default_rng([seed, nx, ny, 7])
    u, w = np.meshgrid(2 * np.pi * np.arange(nx) / nx, 2 * np.pi * np.arange(ny) / ny, indexing="ij")
    v = np.stack([(2 + np.cos(w)) * np.cos(u), (2 + np.cos(w)) * np.sin(u), np.sin(w)], -1).reshape(-1, 3) + rng.uniform(-0.01, 0.01, (nx * ny, 3))
    f = []
    for i in range(nx):
        for j in range(ny):
            a, b, c, d = i * ny + j, ((i + 1) % nx) * ny + j, ((i + 1) % nx) * ny + (j + 1) % ny, i * ny + (j + 1) % ny
            f += [[a, b, c], [a, c, d]]
    return v, np.array(f, np.int32)


def bipyramid(n, seed=0):
    """a closed bipyramid over an n-gon: V = n + 2, both apexes of valence n"""
    rng = np.random.default_rng([seed, n, 3])
    t = 2 * np.pi * np.arange(n) / n
    v = np.concatenate([np.stack([np.cos(t), np.sin(t), np.zeros(n)], 1), [[0, 0, 1.0], [0, 0, -1.0]]]) + rng.uniform(-0.02, 0.02, (n + 2, 3))
    f = [[i, (i + 1) % n, n] for i in range(n)] + [[(i + 1) % n, i, n + 1] for i in range(n)]
    return v, np.array(f, np.int32)


def open_mesh(V, seed=0):
    """an open mesh of exactly V >= 4 vertices: the largest a x b grid below V, the rest as ears on the last row's boundary edges"""
    a = int(np.sqrt(V))
    b = V // a
    v, f = grid(a, b, seed)
    extra = V - a * b
    rng = np.random.default_rng([seed, V, 5])
    ears_v, ears_f = [], []
    for i in range(extra):                                   # boundary edge ((i, b-1), (i+1, b-1)) of the column j = b - 1
        p, q = i * b + b - 1, (i + 1) * b + b - 1
        ears_v.append((v[p] + v[q]) / 2 + [0, 0.8, 0] + rng.uniform(-0.1, 0.1, 3))
        ears_f.append([q, p, a * b + i])
    if extra:
        v, f = np.concatenate([v, ears_v]), np.concatenate([f, np.array(ears_f, np.int32)])
    return v, f


def sphere(levels, seed=0, jitter=0.0):
    """the octahedron split `levels` times at its edge midpoints and pushed onto the unit sphere: F = 8 4^levels, V = 4^(levels + 1) + 2"""
    v = [[1.0, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    f = [[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]
    for _ in range(levels):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                mid[key] = len(v)
                v.append([(v[a][i] + v[b][i]) / 2 for i in range(3)])
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [[a, ab, ca], [ab, b, bc], [ca, bc, c], [ab, bc, ca]]
        f = nf
    v = np.array(v)
    v = v / np.linalg.norm(v, axis=1, keepdims=True)
    if jitter:
        v = v + np.random.default_rng([seed, levels, 11]).uniform(-jitter, jitter, v.shape)
    return v, np.array(f, np.int32)


def shuffled(v, f, seed):
    """the same mesh with its face rows permuted and every face's corners rotated at random (orientation kept)"""
    rng = np.random.default_rng([seed, len(f), 13])
    f = f[rng.permutation(len(f))]
    rot = rng.integers(0, 3, len(f))
    return v, np.stack([f[np.arange(len(f)), (rot + c) % 3] for c in range(3)], 1).astype(f.dtype)


def attributes(V, C, seed=0):
    """(V, C) float32 rows that sum to 1 where C > 0 (a skinning table's shape of numbers), a few entries exactly 0"""
    rng = np.random.default_rng([seed, V, C, 17])
    a = rng.random((V, C)) * (rng.random((V, C)) < 0.4)
    if C:
        a[np.arange(V), rng.integers(0, C, V)] += 0.5
        a = a / a.sum(1, keepdims=True)
    return a.astype(np.float32)


def rigid_transforms(J, seed=0, angle=1.0, shift=0.5):
    """(J,4,4) float64 rotations about random axes by up to `angle` radians, with translations"""
    rng = np.random.default_rng([seed, J, 19])
    A = np.zeros((J, 4, 4))
    for j in range(J):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        t = rng.uniform(-angle, angle)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        A[j, :3, :3] = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K
        A[j, :3, 3] = rng.uniform(-shift, shift, 3)
        A[j, 3, 3] = 1.0
    return A


# ---- the g++ build of csrc/template_bind_math.h ------------------------------------------------------------------------------------------
class PlanStruct(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("V", "F", "E", "reserved")] + [(n, ctypes.c_void_p) for n in PLAN_TABLES]


_LIB = []
_p = gr._p


def lib():
    if not _LIB:
        src = os.path.join(ROOT, "tests", "hostcheck", "template_bind_host.cpp")
        out_dir = os.path.join(ROOT, "tests", "hostcheck", "_build")
        os.makedirs(out_dir, exist_ok=True)
        so = os.path.join(out_dir, "libtemplate_bind_host.so")
        deps = [src, os.path.join(ROOT, "include", "d3ga.h"), os.path.join(ROOT, "d3ga_amd", "csrc", "template_bind_math.h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", so])
        L = ctypes.CDLL(so)
        i32, i64, vp, pp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(PlanStruct)
        L.hc_loop_plan_scratch_bytes.argtypes, L.hc_loop_plan_scratch_bytes.restype = [i32, i32], i64
        L.hc_loop_edge_keys.argtypes = [i32, i32, vp, vp, vp]
        L.hc_loop_plan_build.argtypes = [pp, vp, vp, vp, vp, vp, i64]
        L.hc_loop_subdivide.argtypes = [pp, i32, vp, vp, i32, vp, vp]
        L.hc_loop_faces.argtypes = [pp, vp, vp]
        L.hc_unpose.argtypes = [i32] * 4 + [vp] * 3 + [i32] + [vp] * 3 + [i32, vp, vp]
        _LIB.append(L)
    return _LIB[0]


def host_plan(faces, V):
    """The g++ build -> the oracle's dict (tables cut to E rows).  The sort between the two stages is numpy's stable one."""
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    F = len(f)
    info = np.zeros(4, np.int32)
    keys = np.zeros(3 * F, np.int64)
    assert lib().hc_loop_edge_keys(V, F, _p(f), _p(keys), _p(info[2:3])) == 0
    perm = np.argsort(keys, kind="stable").astype(np.int64)
    sorted_keys = np.ascontiguousarray(keys[perm])
    t = dict(edge_verts=np.full((3 * F, 2), -7, np.int32), edge_opp=np.full((3 * F, 2), -7, np.int32), edge_faces=np.full((3 * F, 2), -7, np.int32),
             edge_boundary=np.full(3 * F, 7, np.uint8), face_edge=np.full((F, 3), -7, np.int32), vert_offsets=np.full(V + 1, -7, np.int32),
             vert_nbr=np.full(6 * F, -7, np.int32), vert_boundary=np.full(V, 7, np.uint8))
    st = PlanStruct(V=V, F=F, E=0, reserved=0, **{k: a.ctypes.data for k, a in t.items()})
    nbytes = lib().hc_loop_plan_scratch_bytes(V, F)
    scratch = gr._aligned(nbytes)
    scratch[:] = 0xEE                                        # the scratch needs no initialisation
    rc = lib().hc_loop_plan_build(ctypes.byref(st), _p(f), _p(sorted_keys), _p(perm), _p(info), _p(scratch), nbytes)
    assert rc == 0, rc
    E = int(info[0])
    out = dict(V=V, F=F, E=E, max_valence=int(info[1]), status=int(info[2]), faces=f.astype(np.int64), _full=t)
    for k, a in t.items():
        out[k] = a[:E] if k.startswith("edge_") else a[:2 * E] if k == "vert_nbr" else a
    return out


def _struct(p):
    full = p.get("_full") or {k: np.ascontiguousarray(p[k]) for k in PLAN_TABLES}
    p["_keep"] = full
    return PlanStruct(V=p["V"], F=p["F"], E=p["E"], reserved=0, **{k: full[k].ctypes.data for k in PLAN_TABLES})


def host_stencil(p, x):
    x = np.ascontiguousarray(x, np.float64)
    D = x.shape[1]
    out = np.full((p["V"] + p["E"], D), np.nan, np.float32)
    if D == 0:
        return out
    beta = beta_table(max(p["max_valence"], 1))
    st, status = _struct(p), np.zeros(1, np.uint32)
    rc = lib().hc_loop_subdivide(ctypes.byref(st), D, _p(x), _p(beta), len(beta), _p(out), _p(status))
    assert rc == 0 and status[0] == 0, (rc, status)
    return out


def host_faces(p):
    f = np.ascontiguousarray(p["faces"], np.int32)
    out = np.full((4 * p["F"], 3), -7, np.int32)
    st = _struct(p)
    assert lib().hc_loop_faces(ctypes.byref(st), _p(f), _p(out)) == 0
    return out


def host_subdivide(vertices, faces, attrs=None, iterations=1):
    v, f = np.asarray(vertices), np.asarray(faces)
    a = None if attrs is None else np.asarray(attrs)
    dtype = f.dtype
    for _ in range(iterations):
        p = host_plan(f, len(v))
        check_status(p["status"])
        v = host_stencil(p, v)
        a = None if a is None else host_stencil(p, a)
        f = host_faces(p)
    return v, f.astype(dtype), a


def host_unpose(vertices, joint_mats, skin, rows=None, offsets=None):
    v, A = np.ascontiguousarray(vertices, np.float64), np.ascontiguousarray(joint_mats, np.float64)
    idx = None
    if isinstance(skin, (tuple, list)):
        idx, w = np.ascontiguousarray(skin[0], np.int32), np.ascontiguousarray(skin[1])
    else:
        w = np.ascontiguousarray(skin)
    assert w.dtype in (np.float32, np.float64)
    r = None if rows is None else np.ascontiguousarray(rows, np.int64)
    b = None if offsets is None else np.ascontiguousarray(offsets, np.float64)
    out, status = np.full((len(v), 3), np.nan, np.float32), np.zeros(1, np.uint32)
    rc = lib().hc_unpose(len(v), len(A), w.shape[0], w.shape[1], _p(v), _p(A), _p(w), int(w.dtype == np.float64), _p(idx), _p(r), _p(b),
                         0 if b is None else len(b), _p(out), _p(status))
    assert rc == 0, rc
    return out, int(status[0])


def same_plan(a, b):
    """every table and every count of two plans equal"""
    for k in ("V", "F", "E", "max_valence", "status"):
        assert a[k] == b[k], (k, a[k], b[k])
    for k in PLAN_TABLES:
        assert np.array_equal(np.asarray(a[k]).reshape(-1), np.asarray(b[k]).reshape(-1)), k
