#!/usr/bin/env python3
"""Generate tests/golden/template_bind_cases.npz -- and nothing else -- by running the reference's OWN functions on the CPU:

    utils.mesh_utils.subdivide_loop(vertices, faces, weights)        as it is
    lib.smplman.Smplman.find_nn(self, template, cage)                on a bare `self` (lbs_module.weights, inflate_cage)
    lib.smplman.Smplman.unpose(self, vertices, T, BS)                on the same `self` (nn_ids), T blended as create_body_model does

Runs only where the reference checkout is present; no test runs it.  The import-stub harness is tools/gen_golden.py's
`install_harness`.  The `trimesh` stub gets content HERE, written from trimesh's documented behaviour, so parity with trimesh
stays UNPINNED:

    geometry.faces_to_edges   rows (a,b), (b,c), (c,a) per face, with the face of every row
    grouping.unique_rows      rows hashed column 0 in the low bits, column 1 above it, then numpy's unique: (first occurrence of
                              every distinct row in ascending hash order, inverse).  For sorted edge rows this is ascending
                              (larger endpoint, smaller endpoint) -- the edge order of record of d3ga_amd/template_bind.py
    grouping.group_rows       the index groups of identical rows, those of `require_count` members as an (n, count) array
    graph.neighbors           per vertex the list of vertices it shares an edge with (ascending here; trimesh's order is a set's)
    graph.connected_components  union-find over the edges (only the reference's non-manifold branch calls it; no case here does)
    Trimesh.vertex_normals    the angle-weighted rule (tests/gauss_init_ref.py::vertex_normals_angle)
    Trimesh.kdtree            scipy.spatial.cKDTree over the CURRENT vertices

float32 vertices and weights go in, as the reference feeds them.  Meshes: a closed jittered octahedron sphere of 128 faces with a
7-column weight table, an open 5 x 4 grid, the two-triangle quad (the boundary quirk).  The generator asserts its own conditions,
so that the reference alone decides every id: in every nearest-vertex query the winner leads the runner-up by a relative margin of
at least 1e-4 of the squared distance (float32 coordinates and float32 distances move a squared distance by less than 1e-6 of
itself at these sizes).  The odd vertex of a boundary edge is equidistant from the edge's ends by construction; those rows are
asserted to be the only ties and `<mesh>_dense_rows` lists the rows that are compared.  Arrays only."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import gen_golden as gg  # noqa: E402
import gauss_init_ref as gr  # noqa: E402
import template_bind_ref as tr  # noqa: E402

OUT = os.path.join(HERE, "..", "tests", "golden", "template_bind_cases.npz")
MARGIN = 1e-4


# ---- trimesh, from its documentation ---------------------------------------------------------------------------------------------------
def faces_to_edges(faces, return_index=False):
    faces = np.asanyarray(faces)
    edges = faces[:, [0, 1, 1, 2, 2, 0]].reshape((-1, 2))
    if return_index:
        return edges, np.tile(np.arange(len(faces)), (3, 1)).T.reshape(-1)
    return edges


def _hash(rows):
    rows = np.asanyarray(rows, np.int64)
    assert rows.ndim == 2 and rows.shape[1] == 2 and rows.min() >= 0 and rows.max() < 2 ** 31
    return rows[:, 0] ^ (rows[:, 1] << 32)


def unique_rows(data):
    _, unique, inverse = np.unique(_hash(data), return_index=True, return_inverse=True)
    return unique, inverse


def group_rows(data, require_count=None):
    h = _hash(data)
    order = np.argsort(h, kind="stable")
    starts = np.nonzero(np.concatenate([[True], h[order][1:] != h[order][:-1]]))[0]
    groups = np.split(order, starts[1:])
    if require_count is None:
        return groups
    keep = [g for g in groups if len(g) == require_count]
    return np.array(keep, np.int64).reshape(-1, require_count)


def neighbors(edges, max_index=None):
    n = int(np.max(edges)) + 1 if max_index is None else int(max_index)
    sets = [set() for _ in range(n)]
    for a, b in np.asarray(edges).tolist():
        sets[a].add(b)
        sets[b].add(a)
    return [sorted(s) for s in sets]


def connected_components(edges, min_len=1, nodes=None):
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    nodes = np.unique(edges) if nodes is None else np.asarray(nodes)
    parent = {int(x): int(x) for x in nodes}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in edges.tolist():
        parent.setdefault(a, a)
        parent.setdefault(b, b)
        parent[find(a)] = find(b)
    groups = {}
    for x in parent:
        groups.setdefault(find(x), []).append(x)
    return [np.array(sorted(g)) for g in groups.values() if len(g) >= min_len]


class Trimesh:
    def __init__(self, vertices, faces, process=False):
        self.vertices, self.faces = np.array(vertices, np.float64), np.array(faces, np.int64)

    @property
    def vertex_normals(self):
        return gr.vertex_normals_angle(self.vertices, self.faces)

    @property
    def kdtree(self):
        from scipy.spatial import cKDTree
        return cKDTree(self.vertices)


STUB = SimpleNamespace(geometry=SimpleNamespace(faces_to_edges=faces_to_edges),
                       grouping=SimpleNamespace(unique_rows=unique_rows, group_rows=group_rows),
                       graph=SimpleNamespace(neighbors=neighbors, connected_components=connected_components), Trimesh=Trimesh)


def margins(template, query, ids):
    best_i, best, second = tr.nearest_margin(template, query)
    assert np.array_equal(best_i, ids)
    return (second - best) / np.maximum(second, 1e-300)


def main():
    gg.install_harness()
    import utils.mesh_utils as mu
    import lib.smplman as sm
    mu.trimesh = STUB
    sm.trimesh = STUB

    meshes = {"sphere": tr.sphere(2, seed=3, jitter=0.03) + (7, 0.02), "grid": tr.grid(5, 4, seed=1) + (3, 0.05), "quad": tr.quad() + (2, 0.0)}
    out = {"names": np.array(list(meshes))}
    for tag, (v, f, C, amount) in meshes.items():
        v32, w32 = v.astype(np.float32), tr.attributes(len(v), C, seed=5)
        f = f.astype(np.int64)
        nv, nf, nw = mu.subdivide_loop(v32.copy(), f.copy(), w32.copy())
        V, E = len(v32), len(nv) - len(v32)
        assert nv.dtype == np.float64 and nw.dtype == np.float64 and nf.shape == (4 * len(f), 3) and nw.shape == (V + E, C)
        # the reference evaluates the odd rows in float32 and the even rows in float64
        assert np.array_equal(nv[V:], nv[V:].astype(np.float32)) and np.array_equal(nw[V:], nw[V:].astype(np.float32))
        rng = np.random.default_rng([9, V])
        cage = (nv[rng.permutation(V + E)[:max(4, (V + E) // 2)]] * (1 + amount + 0.05) + rng.normal(size=(max(4, (V + E) // 2), 3)) * 0.01)
        geo = object.__new__(sm.Smplman)
        geo.lbs_module = SimpleNamespace(weights=torch.from_numpy(w32))
        # the dense template against the template as it is (create_body_model: inflate_cage is 0 there) ...
        geo.inflate_cage = 0
        _, dense_ids = sm.Smplman.find_nn(geo, Trimesh(v32, f), Trimesh(nv, nf))
        m_dense = margins(v32.astype(np.float64), nv, dense_ids)
        # the odd vertex of a BOUNDARY edge is the midpoint of its ends: a tie by construction, which no search pins.  Those rows, and
        # only those, are left out of the dense query (the closed sphere keeps every row)
        plan = tr.plan(f, V)
        tie = np.zeros(V + E, bool)
        tie[V:] = plan["edge_boundary"].astype(bool)
        assert (m_dense[tie] < 1e-6).all()
        dense_rows = np.nonzero(~tie)[0]
        m_dense = m_dense[dense_rows]
        # ... and a cage against the inflated template (create_cage_model)
        geo.inflate_cage = amount
        _, cage_ids = sm.Smplman.find_nn(geo, Trimesh(v32, f), SimpleNamespace(vertices=cage))
        m_cage = margins(tr.inflate(v32, f, amount), cage, cage_ids)
        assert m_dense.min() >= MARGIN and m_cage.min() >= MARGIN, (tag, m_dense.min(), m_cage.min())
        # unpose, as create_body_model calls it: float32 T = skin_weights @ A, vertices and blend offsets in float32
        J = C
        A = torch.from_numpy(tr.rigid_transforms(J, seed=11).astype(np.float32))[None]
        bs = torch.from_numpy((rng.normal(size=(1, V, 3)) * 0.01).astype(np.float32))
        skin = torch.from_numpy(nw).float()
        T = torch.matmul(skin, A.view(1, J, 16)).view(1, -1, 4, 4)
        geo.nn_ids = dense_ids
        vtn = sm.Smplman.unpose(geo, torch.from_numpy(nv)[None].float(), T, bs)
        assert vtn.dtype == torch.float32 and tuple(vtn.shape) == (1, V + E, 3)
        out.update({f"{tag}_vertices": v32, f"{tag}_faces": f.astype(np.int32), f"{tag}_weights": w32, f"{tag}_inflate": np.array(amount),
                    f"{tag}_sub_vertices": nv, f"{tag}_sub_faces": nf.astype(np.int32), f"{tag}_sub_weights": nw,
                    f"{tag}_dense_ids": np.asarray(dense_ids, np.int64), f"{tag}_dense_rows": dense_rows.astype(np.int64), f"{tag}_cage": cage, f"{tag}_cage_ids": np.asarray(cage_ids, np.int64),
                    f"{tag}_joint_mats": A[0].numpy(), f"{tag}_blend_offsets": bs[0].numpy(), f"{tag}_unposed": vtn[0].numpy()})
        print(tag, "V", V, "E", E, "margins", float(m_dense.min()), float(m_cage.min()))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT))


if __name__ == "__main__":
    main()
