"""numpy / plain-Python oracle of part-label transfer (d3ga_amd/mesh_labels.py, csrc/mesh_labels_math.h), written
from the rules and not from the kernels: dictionaries, sets and loops in the order the rules are stated.

    1 neighbours  two different faces are neighbours when they share an undirected edge that occurs in exactly two faces; each
                  edge of a face gives at most one entry; (F,3) int32 padded with -1.  (trimesh's face_adjacency rule; parity
                  with trimesh unpinned.)
    2 view pick   per view and face, the label at the pixel with the largest y W + x among those with pix_to_face == face.
    3 histogram   hist[f, l] += 1 per pick with 0 <= l < L; other labels count nothing and raise the flag; pix_to_face >= F ignored.
    4 majority    over labels 1 .. L-1 the largest count, ties to the smallest label, all zero -> 0.
    5 median      of the neighbours' labels (1: it; 2: (a + b) // 2; 3: the middle; 0: the face's own label).
    6 growth      i qualifies when 0 < #{n in N(i): region[n]} < len(N(i)); mask[j] |= any(qualifies[i] for i in N(j)); n rounds.

Below them the g++ build of csrc/mesh_labels_math.h (tests/hostcheck/mesh_labels_host.cpp), the text the kernels run."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LABELS_MAX = 32


# ---- rule 1 ------------------------------------------------------------------------------------------------------------------------
def adjacency_pairs(faces):
    """(n,2) int64: a row (a, b), a != b, per undirected edge that occurs in exactly two faces"""
    faces = np.asarray(faces).reshape(-1, 3)
    owners = {}
    for f, tri in enumerate(faces.tolist()):
        for e in range(3):
            a, b = tri[e], tri[(e + 1) % 3]
            owners.setdefault((min(a, b), max(a, b)), []).append(f)
    pairs = [fs for _, fs in sorted(owners.items()) if len(fs) == 2 and fs[0] != fs[1]]
    return np.asarray(pairs, np.int64).reshape(-1, 2)


def neighbours_from_pairs(pairs, F):
    """utils/mesh_utils.py::get_neighbours as a table: (F,3) int32, -1 padded"""
    table = np.full((F, 3), -1, np.int32)
    fill = [0] * F
    for a, b in np.asarray(pairs).reshape(-1, 2).tolist():
        for x, y in ((a, b), (b, a)):
            assert fill[x] < 3, "a face has three edges"
            table[x, fill[x]] = y
            fill[x] += 1
    return table


def face_neighbours(faces):
    faces = np.asarray(faces).reshape(-1, 3)
    return neighbours_from_pairs(adjacency_pairs(faces), len(faces))


def same_neighbours(a, b):
    """two tables hold the same entries per face, in any order"""
    return a.shape == b.shape and np.array_equal(np.sort(a, axis=1), np.sort(b, axis=1))


def _ring(table, i):
    F = len(table)
    return [int(n) for n in table[i] if 0 <= n < F]


# ---- rules 2, 3 --------------------------------------------------------------------------------------------------------------------
def view_pick(pix_to_face, labels, F):
    """one view: {face: label of its last pixel in raster order}"""
    pick = {}
    H, W = pix_to_face.shape
    for y in range(H):
        for x in range(W):
            f = int(pix_to_face[y, x])
            if 0 <= f < F:
                pick[f] = int(labels[y, x])
    return pick


def vote(pix_to_face, labels, F, L, hist=None):
    """pix_to_face, labels (B,H,W) -> (hist (F,L) int32, flag): every view on its own"""
    hist = np.zeros((F, L), np.int32) if hist is None else hist.copy()
    flag = 0
    for b in range(len(pix_to_face)):
        for f, l in view_pick(pix_to_face[b], labels[b], F).items():
            if 0 <= l < L:
                hist[f, l] += 1
            else:
                flag = 1
    return hist, flag


# ---- rules 4 - 6 -------------------------------------------------------------------------------------------------------------------
def majority(hist):
    out = np.zeros(len(hist), np.int32)
    for f, row in enumerate(np.asarray(hist)):
        best = max(row[1:].tolist(), default=0)
        if best > 0:
            out[f] = 1 + row[1:].tolist().index(best)
    return out


def histogram(part_per_face, L):
    """the reference's (F, n) array of per-view labels -> (F,L): zeros are no vote (they land in column 0, which no rule reads)"""
    part = np.asarray(part_per_face)
    hist = np.zeros((len(part), L), np.int32)
    for f, row in enumerate(part.tolist()):
        for l in row:
            if 0 <= l < L:
                hist[f, l] += 1
    return hist


def median(table, labels):
    labels = np.asarray(labels)
    out = np.empty(len(table), np.int32)
    for f in range(len(table)):
        ring = sorted(int(labels[n]) for n in _ring(table, f))
        out[f] = labels[f] if not ring else (ring[0] if len(ring) == 1 else (ring[0] + ring[1]) // 2 if len(ring) == 2 else ring[1])
    return out


def grow(table, mask, n_rings):
    F = len(table)
    mask = np.asarray(mask).astype(bool).copy()
    for _ in range(n_rings):
        region = set(np.flatnonzero(mask).tolist())
        qualifies = []
        for i in range(F):
            ring = _ring(table, i)
            count = sum(n in region for n in ring)
            qualifies.append(0 < count < len(ring))
        mask = np.array([bool(mask[j]) or any(qualifies[i] for i in _ring(table, j)) for j in range(F)], bool)
    return mask


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def random_closed_mesh(F, seed):
    """F faces (even, >= 4) of a closed 2-manifold: a tetrahedron grown by random 1 -> 3 face splits, then shuffled"""
    assert F % 2 == 0 and F >= 4
    rng = np.random.default_rng(seed)
    faces = [[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]]
    n_verts = 4
    while len(faces) < F:
        a, b, c = faces.pop(int(rng.integers(len(faces))))
        faces += [[a, b, n_verts], [b, c, n_verts], [c, a, n_verts]]
        n_verts += 1
    faces = np.asarray(faces, np.int64)
    return faces[rng.permutation(len(faces))]


def random_mesh(F, seed):
    """any F >= 1: a closed mesh with faces removed (open borders, faces with 0 .. 3 neighbours)"""
    full = random_closed_mesh(max(4, F + F % 2 + 2), seed)
    return full[:F]


def random_fragments(seed, B, H, W, F, L, bad=0.0):
    """(pix_to_face (B,H,W) int32 with runs, -1 and a few values >= F; labels (B,H,W) int32 in [0, L))"""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(-1, F, (B, H // 3 + 1, W // 5 + 1))
    p2f = np.kron(coarse, np.ones((3, 5), np.int64))[:, :H, :W]
    noise = rng.random((B, H, W)) < 0.3
    p2f = np.where(noise, rng.integers(-1, F + 2, (B, H, W)), p2f).astype(np.int32)
    labels = rng.integers(0, L, (B, H, W)).astype(np.int32)
    if bad:
        wrong = rng.random((B, H, W)) < bad
        labels[wrong] = rng.choice(np.array([-1, L, L + 7, 255], np.int32), int(wrong.sum()))
    return p2f, labels


# ---- the g++ build of csrc/mesh_labels_math.h ---------------------------------------------------------------------------------------
_LIB = []
EVERY_PIXEL = 1                                              # D3GA_LABEL_EVERY_PIXEL (include/d3ga.h)


def lib():
    if not _LIB:
        src = os.path.join(ROOT, "tests", "hostcheck", "mesh_labels_host.cpp")
        out_dir = os.path.join(ROOT, "tests", "hostcheck", "_build")
        os.makedirs(out_dir, exist_ok=True)
        so = os.path.join(out_dir, "libmesh_labels_host.so")
        deps = [src, os.path.join(ROOT, "include", "d3ga.h"), os.path.join(ROOT, "d3ga_amd", "csrc", "mesh_labels_math.h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", src, "-o", so])
        L = ctypes.CDLL(so)
        i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
        L.hc_label_vote.argtypes = [i32] * 5 + [vp, vp, i32, i64, i64, vp, vp, vp, i32, ctypes.POINTER(i64)]
        L.hc_label_majority.argtypes = [i32, i32, vp, vp]
        L.hc_label_median.argtypes = [i32, vp, vp, vp]
        L.hc_label_grow.argtypes = [i32, i32, vp, vp, vp, vp]
        _LIB.append(L)
    return _LIB[0]


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_vote(pix_to_face, labels, F, L, hist=None, flags=0):
    """The g++ build on numpy arrays: pix_to_face (B,H,W) int32 contiguous; labels (B,H,W) or (B,1,H,W), int32 or uint8, any row
    pitch and frame stride (views are addressed through their strides).  -> (hist, status, keys sent); asserts that the cells are
    all zero afterwards."""
    B, H, W = pix_to_face.shape
    assert pix_to_face.dtype == np.int32 and pix_to_face.flags.c_contiguous
    if labels.ndim == 4:
        labels = labels[:, 0]
    assert labels.dtype in (np.int32, np.uint8) and (W == 1 or labels.strides[2] == labels.itemsize)
    hist = np.zeros((F, L), np.int32) if hist is None else np.ascontiguousarray(hist, np.int32).copy()
    cells = np.zeros((B, F), np.uint32)
    status, sent = np.zeros(1, np.uint32), ctypes.c_int64(-1)
    pitch = labels.strides[1] if H > 1 else W * labels.itemsize
    st = lib().hc_label_vote(B, F, L, H, W, _p(pix_to_face), _p(labels), int(labels.dtype == np.uint8), pitch, labels.strides[0], _p(cells),
                             _p(hist), _p(status), flags, ctypes.byref(sent))
    assert st == 0, st
    assert not cells.any()
    return hist, int(status[0]), sent.value


def host_majority(hist):
    hist = np.ascontiguousarray(hist, np.int32)
    out = np.full(len(hist), -9, np.int32)
    assert lib().hc_label_majority(hist.shape[0], hist.shape[1], _p(hist), _p(out)) == 0
    return out


def host_median(table, labels):
    table, labels = np.ascontiguousarray(table, np.int32), np.ascontiguousarray(labels, np.int32)
    out = np.full(len(table), -9, np.int32)
    assert lib().hc_label_median(len(table), _p(table), _p(labels), _p(out)) == 0
    return out


def host_grow(table, mask, n_rings):
    table, mask = np.ascontiguousarray(table, np.int32), np.ascontiguousarray(mask).astype(np.uint8)
    out, scratch = np.full(len(table), 7, np.uint8), np.full(2 * len(table), 7, np.uint8)
    assert lib().hc_label_grow(len(table), n_rings, _p(table), _p(mask), _p(out), _p(scratch)) == 0
    return out.astype(bool)
