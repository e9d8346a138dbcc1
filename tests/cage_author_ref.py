"""The oracle of cage surface authoring (d3ga_amd/cage_author.py) in numpy and scipy, restated from the rules and
not from the header's code: the 13-axis triangle / cube test in the header's operation order, vectorised over a triangle's voxels;
`scipy.ndimage.binary_fill_holes`; marching tetrahedra as a plain Python loop over the mixed cells, oriented by a float test on
the geometry and numbered by sorting edge keys; both smoothers over `scipy.sparse` Laplacians; parts by
`scipy.sparse.csgraph.connected_components`.  Parity with trimesh, mcubes and open3d is unpinned (the project depends on none of them).

Below them the g++ build of csrc/cage_author_math.h (tests/hostcheck/cage_author_host.cpp), the text the kernels run, and the
shapes the tests share.  Dense grids are bool (D,D,D) indexed [x,y,z]."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import scipy.ndimage as ndi
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

import gauss_init_ref as gr
import template_bind_ref as tr

ROOT = tr.ROOT
STATUS_RANGE, STATUS_ISOLATED, STATUS_ZERO_EDGE = 1, 2, 4    # D3GA_CAGE_STATUS_* (include/d3ga.h)
FILL_BEGIN, FILL_ROUND, FILL_FINISH = 0, 1, 2
IMPROVED, TAUBIN = 0, 1
PARTS_BEGIN, PARTS_ROUND = 0, 1
TETS = [[0] + list(itertools.accumulate((1 << a for a in p), lambda x, y: x | y)) for p in itertools.permutations(range(3))]
TYPE_OFFSETS = (1, 2, 4, 3, 5, 6, 7)                         # x, y, z, xy, xz, yz, xyz
same_bits = gr.same_bits
_p = gr._p


def pitch(radius):
    return 1.0 / (radius + 0.1)


# ---- 1 surface voxels ------------------------------------------------------------------------------------------------------------------
def _separates(ax, ay, az, v, h):
    p = [(ax * v[:, 3 * i] + ay * v[:, 3 * i + 1]) + az * v[:, 3 * i + 2] for i in range(3)]
    r = h * ((np.abs(ax) + np.abs(ay)) + np.abs(az))
    return (np.minimum(np.minimum(p[0], p[1]), p[2]) > r) | (np.maximum(np.maximum(p[0], p[1]), p[2]) < -r)


def tri_box(t, centres, h):
    """t (9,), centres (n,3) -> (n,) bool: the triangle meets the closed cube of half side h at each centre"""
    v = t[None, :] - np.tile(centres, 3)
    zero, one = np.zeros(len(v)), np.ones(len(v))
    sep = _separates(one, zero, zero, v, h) | _separates(zero, one, zero, v, h) | _separates(zero, zero, one, v, h)
    f = np.concatenate([v[:, 3:6] - v[:, 0:3], v[:, 6:9] - v[:, 3:6], v[:, 0:3] - v[:, 6:9]], 1)
    for j in range(3):
        fx, fy, fz = f[:, 3 * j], f[:, 3 * j + 1], f[:, 3 * j + 2]
        sep |= _separates(zero, -fz, fy, v, h) | _separates(fz, zero, -fx, v, h) | _separates(-fy, fx, zero, v, h)
    sep |= _separates(f[:, 1] * f[:, 5] - f[:, 2] * f[:, 4], f[:, 2] * f[:, 3] - f[:, 0] * f[:, 5], f[:, 0] * f[:, 4] - f[:, 1] * f[:, 3], v, h)
    return ~sep


def surface(vertices, faces, radius):
    """the surface voxels of a mesh -> dense bool (D,D,D); every voxel within two of a triangle's box is tried"""
    v, f = np.asarray(vertices, np.float64), np.asarray(faces, np.int64).reshape(-1, 3)
    D, pt = 2 * radius + 1, pitch(radius)
    out = np.zeros((D, D, D), bool)
    for tri in v[f]:
        lo = np.clip(np.floor(np.clip(tri.min(0) / pt, -2 * D, 2 * D) + radius + 0.5).astype(np.int64) - 2, 0, D)
        hi = np.clip(np.floor(np.clip(tri.max(0) / pt, -2 * D, 2 * D) + radius + 0.5).astype(np.int64) + 2, -1, D - 1)
        if (lo > hi).any():
            continue
        idx = np.stack(np.meshgrid(*(np.arange(a, b + 1) for a, b in zip(lo, hi)), indexing="ij"), -1).reshape(-1, 3)
        hit = tri_box(tri.reshape(9), (idx - radius).astype(np.float64) * pt, pt / 2.0)
        out[tuple(idx[hit].T)] = True
    return out


def point_triangle_distance(points, triangles):
    """points (n,3), triangles (m,3,3) -> (n,) the distance of every point to the nearest triangle (Ericson's closest point)"""
    best = np.full(len(points), np.inf)
    for a, b, c in triangles:
        ab, ac, ap = b - a, c - a, points - a
        d1, d2 = ap @ ab, ap @ ac
        bp = points - b
        d3, d4 = bp @ ab, bp @ ac
        cp = points - c
        d5, d6 = cp @ ab, cp @ ac
        va, vb, vc = d3 * d6 - d5 * d4, d5 * d2 - d1 * d6, d1 * d4 - d3 * d2
        with np.errstate(all="ignore"):
            denom = va + vb + vc
            q = a + ab * (vb / denom)[:, None] + ac * (vc / denom)[:, None]                     # inside the face
            q = np.where(((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0))[:, None], b + (c - b) * ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[:, None], q)
            q = np.where(((vb <= 0) & (d2 >= 0) & (d6 <= 0))[:, None], a + ac * (d2 / (d2 - d6))[:, None], q)
            q = np.where(((vc <= 0) & (d1 >= 0) & (d3 <= 0))[:, None], a + ab * (d1 / (d1 - d3))[:, None], q)
        q = np.where(((d6 >= 0) & (d5 <= d6))[:, None], c, q)
        q = np.where(((d3 >= 0) & (d4 <= d3))[:, None], b, q)
        q = np.where(((d1 <= 0) & (d2 <= 0))[:, None], a, q)
        if np.linalg.norm(np.cross(ab, ac)) == 0:                                               # no area: the nearest of its three edges' ends and midpoints is not enough
            q = _closest_on_segments(points, (a, b, c))
        best = np.minimum(best, np.linalg.norm(points - q, axis=1))
    return best


def _closest_on_segments(points, corners):
    best, out = np.full(len(points), np.inf), np.zeros_like(points)
    for i in range(3):
        a, d = corners[i], corners[(i + 1) % 3] - corners[i]
        dd = d @ d
        t = np.clip((points - a) @ d / dd, 0, 1) if dd > 0 else np.zeros(len(points))
        q = a + t[:, None] * d
        dist = np.linalg.norm(points - q, axis=1)
        out = np.where((dist < best)[:, None], q, out)
        best = np.minimum(best, dist)
    return out


# ---- 2 fill ---------------------------------------------------------------------------------------------------------------------------
def fill(dense):
    return ndi.binary_fill_holes(dense)


# ---- 3 isosurface ---------------------------------------------------------------------------------------------------------------------
def isosurface(dense, centre=(0.0, 0.0, 0.0), scale=(1.0, 1.0, 1.0)):
    """marching tetrahedra by the rule of DESIGN.md 4.4u -> (vertices (n,3) float32, faces (m,3) int32, edges (n,2,3) the grid
    corners each vertex lies between)"""
    D = dense.shape[0]
    P, radius = D + 1, (D - 1) // 2
    pad = np.zeros((D + 2,) * 3, bool)
    pad[1:-1, 1:-1, 1:-1] = dense                             # lattice point p is pad[p]: grid corner p - 1
    corners = np.stack([pad[(b & 1):(b & 1) + P, ((b >> 1) & 1):((b >> 1) & 1) + P, (b >> 2):(b >> 2) + P] for b in range(8)])
    cells = np.argwhere(corners.any(0) & ~corners.all(0))
    cells = cells[np.argsort((cells[:, 2] * P + cells[:, 1]) * P + cells[:, 0], kind="stable")]
    type_of = {off: t for t, off in enumerate(TYPE_OFFSETS)}
    bits = lambda b: np.array([b & 1, (b >> 1) & 1, b >> 2])
    keys = []                                                # one per face corner: (linear index of the lower end) * 7 + type
    for cell in cells:
        val = [bool(pad[tuple(cell + bits(b))]) for b in range(8)]
        for t in TETS:
            ins, outs = [c for c in t if val[c]], [c for c in t if not val[c]]
            if not ins or not outs:
                continue
            if len(ins) == 1 or len(outs) == 1:
                s = ins[0] if len(ins) == 1 else outs[0]
                tris = [[(s, o) for o in t if o != s]]
            else:
                (a, b), (c, d) = ins, outs
                q = [(a, c), (a, d), (b, d), (b, c)]
                tris = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
            for tri in tris:
                p = [(bits(a) + bits(b)) / 2.0 for a, b in tri]
                towards = np.mean([bits(c) for c in outs], 0) - np.mean([bits(c) for c in ins], 0)
                if np.dot(np.cross(p[1] - p[0], p[2] - p[0]), towards) < 0:
                    tri = [tri[0], tri[2], tri[1]]
                for a, b in tri:
                    lower = cell + bits(min(a, b))
                    keys.append(((lower[2] * P + lower[1]) * P + lower[0]) * 7 + type_of[a ^ b])
    keys = np.array(keys, np.int64)
    unique = np.unique(keys)
    faces = np.searchsorted(unique, keys).astype(np.int32).reshape(-1, 3)
    lin, typ = unique // 7, unique % 7
    lower = np.stack([lin % P, (lin // P) % P, lin // (P * P)], 1) - 1
    upper = lower + np.array([bits(TYPE_OFFSETS[t]) for t in typ]).reshape(-1, 3)
    x = (lower + upper) / 2.0
    vertices = (((x / radius - 1.0) + np.asarray(centre, np.float64)) / np.asarray(scale, np.float64)).astype(np.float32)
    return vertices, faces, np.stack([lower, upper], 1)


def edge_census(faces):
    """-> (every undirected edge is in exactly two faces, every directed edge appears once, the number of undirected edges)"""
    f = np.asarray(faces, np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    directed = np.unique(d, axis=0, return_counts=True)[1]
    undirected = np.unique(np.sort(d, 1), axis=0, return_counts=True)[1]
    return bool((undirected == 2).all()), bool((directed == 1).all()), len(undirected)


def signed_volume(vertices, faces):
    v = np.asarray(vertices, np.float64)
    a, b, c = (v[np.asarray(faces)[:, k]] for k in range(3))
    return float((a * np.cross(b, c)).sum() / 6.0)


# ---- 4 smoothers ------------------------------------------------------------------------------------------------------------------------
def _edges(faces):
    f = np.asarray(faces, np.int64)
    e = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1), axis=0)
    return np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]])


def vertex_normals(v, f, perturb=None):
    """angle-weighted vertex normals; perturb: a generator -- every acos moved one ulp up or down at random"""
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    fn /= np.maximum(np.linalg.norm(fn, axis=1, keepdims=True), 1e-12)
    N = np.zeros_like(v)
    for c in range(3):
        a, b = v[f[:, (c + 1) % 3]] - v[f[:, c]], v[f[:, (c + 2) % 3]] - v[f[:, c]]
        a /= np.maximum(np.linalg.norm(a, axis=1, keepdims=True), 1e-12)
        b /= np.maximum(np.linalg.norm(b, axis=1, keepdims=True), 1e-12)
        ang = np.arccos(np.clip((a * b).sum(1), -1, 1))
        if perturb is not None:
            ang = np.nextafter(ang, ang + perturb.choice([-1.0, 1.0], len(ang)))
        np.add.at(N, f[:, c], fn * ang[:, None])
    return N / np.maximum(np.linalg.norm(N, axis=1, keepdims=True), 1e-12)


def smooth_improved(vertices, faces, num_iter=25, lbd=0.25, perturb=None, details=False):
    """-> float32 (V,3); details: also the float64 result, the `inner >= 0` branches (num_iter, V) and the smallest |inner| / |dot|"""
    v, f = np.array(vertices, np.float64), np.asarray(faces, np.int64)
    V = len(v)
    I, J = _edges(f)
    branches, margin = [], np.inf
    for _ in range(num_iter):
        w = 1.0 / np.linalg.norm(v[I] - v[J], axis=1)
        L = sp.csr_matrix((w, (I, J)), shape=(V, V))
        L = sp.diags(1.0 / np.asarray(L.sum(1)).reshape(-1)) @ L
        dot = L @ v - v
        N = vertex_normals(v, f, perturb)
        inner = (dot * N).sum(1, keepdims=True)
        H = np.linalg.norm(dot, axis=1, keepdims=True)
        branches.append(inner[:, 0] >= 0)
        margin = min(margin, float((np.abs(inner) / H).min()))
        v = v + lbd * np.where(inner >= 0, H * N, dot - inner * N)
    return (v.astype(np.float32), v, np.array(branches), margin) if details else v.astype(np.float32)


def smooth_taubin(vertices, faces, iterations=10, lam=0.5, mu=-0.53):
    v, f = np.array(vertices, np.float64), np.asarray(faces, np.int64)
    I, J = _edges(f)
    A = sp.csr_matrix((np.ones(len(I)), (I, J)), shape=(len(v), len(v)))
    M = sp.diags(1.0 / np.asarray(A.sum(1)).reshape(-1)) @ A
    for _ in range(iterations):
        v = v + lam * (M @ v - v)
        v = v + mu * (M @ v - v)
    return v.astype(np.float32)


# ---- 5 parts --------------------------------------------------------------------------------------------------------------------------
def components(faces):
    """-> (F,) int32: the smallest face index of every face's part (faces that share an edge are adjacent)"""
    f = np.asarray(faces, np.int64)
    F = len(f)
    d = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    owner = np.tile(np.arange(F), 3)
    order = np.lexsort((d[:, 1], d[:, 0]))
    d, owner = d[order], owner[order]
    same = (d[1:] == d[:-1]).all(1)
    A = sp.csr_matrix((np.ones(same.sum()), (owner[:-1][same], owner[1:][same])), shape=(F, F))
    part = connected_components(A, directed=False)[1]
    smallest = np.full(part.max() + 1, F, np.int64)
    np.minimum.at(smallest, part, np.arange(F))
    return smallest[part].astype(np.int32)


def keep_components(vertices, faces, min_faces=70, drop_unreferenced=True, labels=None):
    v, f = np.asarray(vertices), np.asarray(faces)
    labels = components(f) if labels is None else labels
    f = f[np.bincount(labels, minlength=len(f))[labels] >= min_faces]
    if len(f) and signed_volume(v, f) < 0:
        f = f[:, [0, 2, 1]]
    if drop_unreferenced:
        used = np.zeros(len(v), bool)
        used[f.reshape(-1)] = True
        v, f = v[used], (np.cumsum(used) - 1)[f]
    return v, f.astype(np.int32)


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------
def lattice(radius):
    D = 2 * radius + 1
    return np.mgrid[:D, :D, :D] - radius


def ball(radius, r=None, centre=(0, 0, 0)):
    x, y, z = lattice(radius)
    return (x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2 <= (0.73 * radius if r is None else r) ** 2


def ellipsoid_grid(radius=8):
    x, y, z = lattice(radius)
    return (x / 1.0) ** 2 + (y / 0.8) ** 2 + (z / 0.6) ** 2 <= (6.3 * radius / 8) ** 2


def torus_grid(radius=10):
    x, y, z = lattice(radius)
    return (np.sqrt(x ** 2 + y ** 2) - 0.6 * radius) ** 2 + z ** 2 <= (0.26 * radius) ** 2


def shell_grid(radius=10):
    x, y, z = lattice(radius)
    d = x ** 2 + y ** 2 + z ** 2
    return (d <= (0.82 * radius) ** 2) & (d >= (0.61 * radius) ** 2)


def bowl_grid(radius=10):
    g = shell_grid(radius)
    g[:, :, radius + 2:] = False                             # the upper part cut away: open to the outside
    return g


def serpentine_grid(radius=10):
    """a solid block with a one-voxel corridor that winds from the border to a chamber: the sweeps need several rounds"""
    D = 2 * radius + 1
    g = np.zeros((D, D, D), bool)
    g[2:-2, 2:-2, 2:-2] = True
    z = radius
    for k, y in enumerate(range(3, D - 3, 2)):               # rows of the corridor, joined alternately at either end
        g[3:D - 3, y, z] = False
        if y + 2 < D - 3:
            g[D - 4 if k % 2 == 0 else 3, y + 1, z] = False
    g[3, 0:3, z] = False                                     # the mouth
    return g


def voxel_cases(radius):
    """(name, vertices float64, faces int32): the shapes of the voxeliser's edge cases at this radius"""
    pt = pitch(radius)
    tri = np.array([[0, 1, 2]], np.int32)
    sv, sf = tr.sphere(2, seed=radius, jitter=0.01)
    yield "a triangle inside one voxel", np.array([[0.1, 0.2, -0.1], [0.3, 0.1, 0.1], [0.2, 0.3, 0.2]]) * pt + np.array([2.0, -1.0, 3.0]) * pt, tri
    yield "a triangle larger than the grid", np.array([[-5.0, -4.0, 0.013], [6.0, -3.0, 0.021], [0.5, 7.0, -0.017]]), tri
    yield "a mesh partly outside the grid", sv * 0.8 + np.array([0.6, 0.1, -0.2]), sf
    yield "a mesh that touches the border", sv * 1.0, sf
    yield "a zero-area triangle", np.array([[0.0, 0.0, 0.0], [0.3, 0.2, 0.1], [0.6, 0.4, 0.2], [0.11, -0.32, 0.2]]), np.array([[0, 1, 2], [3, 3, 3]], np.int32)
    yield "a vertex on a voxel face", np.array([[0.5 * pt, 0.0, 0.0], [0.5 * pt, 0.2 * pt, 0.1 * pt], [0.5 * pt, -0.1 * pt, 0.3 * pt]]), tri
    yield "a sphere", sv * 0.6, sf


def counted_grid(radius, singles, pairs):
    """`singles` lone voxels and `pairs` x-adjacent pairs, none touching another: 14 singles + 26 pairs crossed edges.  A lone voxel
    ends 14 Kuhn edges; a crossed-edge count is always even (14 per occupied lattice point less 2 per edge inside)."""
    D = 2 * radius + 1
    slots = [(1 + 3 * i, 1 + 3 * j, 1 + 3 * k) for k in range((D - 1) // 3) for j in range((D - 1) // 3) for i in range((D - 1) // 3)]
    assert singles + pairs <= len(slots)
    g = np.zeros((D, D, D), bool)
    for n, (x, y, z) in enumerate(slots[:singles + pairs]):
        g[x, y, z] = True
        if n >= singles:
            g[x + 1, y, z] = True
    return g


def mesh_of(dense, seed=None, jitter=0.0):
    """the oracle's isosurface of a grid as float64 vertices (jittered for general position) and int32 faces"""
    v, f, _ = isosurface(dense)
    v = v.astype(np.float64)
    if jitter:
        v = v + np.random.default_rng(seed).normal(0, jitter, v.shape)
    return v, f


def capsule_figure(seed=3, r=20, through_host_build=False):
    """a closed figure of capsule limbs (trunk, two arms, two legs, a head): the union's surface from a (2 r + 1)^3 grid, jittered"""
    x, y, z = (a / r for a in lattice(r))
    def capsule(p, q, rad):
        p, q = np.array(p, float), np.array(q, float)
        d = q - p
        t = np.clip(((x - p[0]) * d[0] + (y - p[1]) * d[1] + (z - p[2]) * d[2]) / (d @ d), 0, 1)
        return (x - p[0] - t * d[0]) ** 2 + (y - p[1] - t * d[1]) ** 2 + (z - p[2] - t * d[2]) ** 2 <= rad ** 2
    g = capsule((0, 0, -0.1), (0, 0, 0.4), 0.2) | capsule((0, 0, 0.62), (0, 0, 0.66), 0.13)
    g |= capsule((0.15, 0, 0.4), (0.6, 0, 0.15), 0.08) | capsule((-0.15, 0, 0.4), (-0.6, 0, 0.15), 0.08)
    g |= capsule((0.1, 0, -0.15), (0.22, 0, -0.75), 0.1) | capsule((-0.1, 0, -0.15), (-0.22, 0, -0.75), 0.1)
    if through_host_build:                                   # the same surface, without the Python loop
        v, f = host_isosurface(g)
        return v.astype(np.float64) + np.random.default_rng(seed).normal(0, 0.002 * 20 / r, v.shape), f
    return mesh_of(g, seed, 0.002)


# ---- the g++ build of csrc/cage_author_math.h -------------------------------------------------------------------------------------------
class GridStruct(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("radius", "D", "W", "reserved")] + [("bits", ctypes.c_void_p)]


class IsoStruct(ctypes.Structure):
    _fields_ = [("n_vertices", ctypes.c_int32), ("n_faces", ctypes.c_int32), ("centre", ctypes.c_double * 3), ("scale", ctypes.c_double * 3),
                ("vertices", ctypes.c_void_p), ("faces", ctypes.c_void_p)]


class SmoothStruct(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int32), ("iterations", ctypes.c_int32), ("lam", ctypes.c_double), ("mu", ctypes.c_double)] + \
               [(n, ctypes.c_void_p) for n in ("x", "work", "normals", "faces", "csr_offsets", "csr_faces", "out", "status")]


_LIB = []


def lib():
    if not _LIB:
        src = os.path.join(ROOT, "tests", "hostcheck", "cage_author_host.cpp")
        out_dir = os.path.join(ROOT, "tests", "hostcheck", "_build")
        os.makedirs(out_dir, exist_ok=True)
        so = os.path.join(out_dir, "libcage_author_host.so")
        deps = [src, os.path.join(ROOT, "include", "d3ga.h")] + [os.path.join(ROOT, "d3ga_amd", "csrc", h) for h in ("cage_author_math.h", "gauss_init_math.h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", so])
        L = ctypes.CDLL(so)
        i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
        gp, pp = ctypes.POINTER(GridStruct), ctypes.POINTER(tr.PlanStruct)
        L.hc_cage_voxelize.argtypes = [gp, i32, i32, vp, vp, vp]
        L.hc_cage_fill.argtypes = [gp, i32, vp, vp, vp]
        L.hc_cage_iso_scratch_bytes.argtypes, L.hc_cage_iso_scratch_bytes.restype = [i32], i64
        L.hc_cage_iso_count.argtypes = [gp, vp, i64, vp]
        L.hc_cage_iso_emit.argtypes = [gp, ctypes.POINTER(IsoStruct), vp, i64]
        L.hc_cage_smooth.argtypes = [pp, ctypes.POINTER(SmoothStruct)]
        L.hc_cage_components.argtypes = [pp, i32, vp, vp]
        _LIB.append(L)
    return _LIB[0]


def pack(dense):
    """dense bool (D,D,D) [x,y,z] -> the bit array (D, D, W) uint64 [z][y][x >> 6]"""
    D = dense.shape[0]
    W = (D + 63) // 64
    zyx = np.zeros((D, D, 64 * W), np.uint64)
    zyx[:, :, :D] = dense.transpose(2, 1, 0)
    return np.ascontiguousarray((zyx.reshape(D, D, W, 64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64))


def unpack(bits, D):
    zyx = ((bits[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).reshape(D, D, -1)
    assert not zyx[:, :, D:].any()                           # nothing beyond the row's end
    return np.ascontiguousarray(zyx[:, :, :D].transpose(2, 1, 0)).astype(bool)


def _grid(bits, radius):
    D = 2 * radius + 1
    return GridStruct(radius=radius, D=D, W=(D + 63) // 64, reserved=0, bits=bits.ctypes.data)


def host_surface(vertices, faces, radius):
    v, f = np.ascontiguousarray(vertices, np.float64), np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    D = 2 * radius + 1
    bits = np.full((D, D, (D + 63) // 64), 0xEEEEEEEEEEEEEEEE, np.uint64)     # the grid needs no initialisation
    status = np.zeros(1, np.uint32)
    g = _grid(bits, radius)
    rc = lib().hc_cage_voxelize(ctypes.byref(g), len(v), len(f), _p(v), _p(f), _p(status))
    assert rc == 0, rc
    return unpack(bits, D), int(status[0])


def host_fill(dense):
    """-> (filled dense, rounds)"""
    D = dense.shape[0]
    surface_bits = pack(dense)
    outside, filled = np.full_like(surface_bits, 0xEE), np.full_like(surface_bits, 0xEE)
    g = _grid(surface_bits, (D - 1) // 2)
    assert lib().hc_cage_fill(ctypes.byref(g), FILL_BEGIN, _p(outside), None, None) == 0
    rounds = 0
    while True:
        changed = np.zeros(1, np.int32)
        assert lib().hc_cage_fill(ctypes.byref(g), FILL_ROUND, _p(outside), None, _p(changed)) == 0
        rounds += 1
        if not changed[0]:
            break
    assert lib().hc_cage_fill(ctypes.byref(g), FILL_FINISH, _p(outside), _p(filled), None) == 0
    return unpack(filled, D), rounds


def host_isosurface(dense, centre=(0.0, 0.0, 0.0), scale=(1.0, 1.0, 1.0)):
    D = dense.shape[0]
    radius = (D - 1) // 2
    bits = pack(dense)
    g = _grid(bits, radius)
    nbytes = lib().hc_cage_iso_scratch_bytes(radius)
    scratch = gr._aligned(nbytes)
    scratch[:] = 0xEE
    counts = np.zeros(2, np.int64)
    assert lib().hc_cage_iso_count(ctypes.byref(g), _p(scratch), nbytes, _p(counts)) == 0
    v, f = np.full((counts[0], 3), np.nan, np.float32), np.full((counts[1], 3), -7, np.int32)
    if counts[0] and counts[1]:
        o = IsoStruct(n_vertices=int(counts[0]), n_faces=int(counts[1]), centre=(ctypes.c_double * 3)(*centre), scale=(ctypes.c_double * 3)(*scale),
                      vertices=v.ctypes.data, faces=f.ctypes.data)
        assert lib().hc_cage_iso_emit(ctypes.byref(g), ctypes.byref(o), _p(scratch), nbytes) == 0
    return v, f


def vertex_faces(faces, V):
    f = np.asarray(faces, np.int64).reshape(-1)
    order = np.argsort(f, kind="stable")
    offsets = np.zeros(V + 1, np.int32)
    offsets[1:] = np.cumsum(np.bincount(f, minlength=V))
    return offsets, np.ascontiguousarray(order // 3, np.int32)


def host_smooth(mode, vertices, faces, iterations, lam, mu=0.0, plan=None):
    """-> (float32 (V,3), status)"""
    x, f = np.array(vertices, np.float64, order="C"), np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    V = len(x)
    p = plan or tr.plan(f, V)
    st = tr._struct(p)
    work, normals, out, status = np.full_like(x, np.nan), np.full_like(x, np.nan), np.full((V, 3), np.nan, np.float32), np.zeros(1, np.uint32)
    offsets, idx = vertex_faces(f, V)
    d = SmoothStruct(mode=mode, iterations=iterations, lam=lam, mu=mu, x=x.ctypes.data, work=work.ctypes.data, normals=normals.ctypes.data,
                     faces=f.ctypes.data, csr_offsets=offsets.ctypes.data, csr_faces=idx.ctypes.data, out=out.ctypes.data, status=status.ctypes.data)
    rc = lib().hc_cage_smooth(ctypes.byref(st), ctypes.byref(d))
    assert rc == 0, rc
    return out, int(status[0])


def host_components(faces, V, plan=None):
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    p = plan or tr.plan(f, V)
    st = tr._struct(p)
    label = np.full(len(f), -7, np.int32)
    assert lib().hc_cage_components(ctypes.byref(st), PARTS_BEGIN, _p(label), None) == 0
    while True:
        changed = np.zeros(1, np.int32)
        assert lib().hc_cage_components(ctypes.byref(st), PARTS_ROUND, _p(label), _p(changed)) == 0
        if not changed[0]:
            return label


def host_chain(prepared, faces, radius, centre, scale):
    """the stages of `cage_processor` after `prepare`, through the g++ build -> (vertices float32, faces int32, the filled grid)"""
    grid, _ = host_fill(host_surface(prepared, faces, radius)[0])
    v, f = host_isosurface(grid, centre, (scale, scale, 1.0))
    v, st = host_smooth(IMPROVED, v, f, 25, 0.25)
    assert st == 0
    v, st = host_smooth(TAUBIN, v, f, 10, 0.5, -0.53)
    assert st == 0
    v, f = keep_components(v, f, 70, True, host_components(f, len(v)))
    return v, f, grid
