#!/usr/bin/env python3
"""Generate tests/golden/mesh_labels_cases.npz -- and nothing else -- by running the reference's OWN functions on the CPU:

    utils.mesh_utils.median_filter_mesh(mesh, labels)              mesh duck-typed: .faces, .face_adjacency
    lib.segmentation.Segmenter.majority_vote(None, part_per_face)
    lib.cage.CageBase.grow_mask_region(None, mesh, mask, n_rings)
    lib.segmentation.Renderer.forward(fake_self, None, vertices, faces, images)   fake_self.rasterizer returns prepared fragments; B = 1

Runs only where the reference checkout is present; no test runs it.  The import-stub harness is tools/gen_golden.py's
`install_harness`.  trimesh is one of its stubs: `face_adjacency` is built HERE by trimesh's documented rule (tests/mesh_labels_ref.py
::adjacency_pairs -- a pair per undirected edge that occurs in exactly two faces) and recorded with the case, so parity with
trimesh is unpinned.

Arrays only.  Three meshes: `grid`, an open 6 x 5 grid of 60 triangles (faces with 1 and 2 neighbours at its corners and border);
`octa`, a twice-subdivided octahedron of 128 faces (closed); `fins`, a 3 x 2 grid with a fin on an interior edge (an edge in three
faces) and a pair of faces that share two edges.  Per mesh: faces, adjacency, face labels in 0..4 and their median; (F, 9) per-view
labels with ties and all-zero rows and their majority; four masks and their growth by 1, 2 and 10 rings; fragments of 23 x 31 and
16 x 64 with -1, label images in 0..4 and what Renderer.forward scatters onto the faces."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import gen_golden as gg  # noqa: E402
import mesh_labels_ref as mr  # noqa: E402

OUT = os.path.join(HERE, "..", "tests", "golden", "mesh_labels_cases.npz")
SIZES = ((23, 31), (16, 64))
RINGS = (1, 2, 10)


def grid_mesh(nx, ny, first=0):
    vid = lambda i, j: first + j * (nx + 1) + i
    faces = []
    for j in range(ny):
        for i in range(nx):
            a, b, c, d = vid(i, j), vid(i + 1, j), vid(i + 1, j + 1), vid(i, j + 1)
            faces += [[a, b, c], [a, c, d]]
    return np.asarray(faces, np.int64)


def octahedron(levels):
    verts = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    faces = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    for _ in range(levels):
        mid, out = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                mid[key] = len(verts)
                verts.append(tuple((np.asarray(verts[a]) + np.asarray(verts[b])) / 2))
            return mid[key]
        for a, b, c in faces:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            out += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        faces = out
    return np.asarray(faces, np.int64)


def fins_mesh():
    faces = grid_mesh(3, 2).tolist()                         # 12 faces, vertices 0 .. 11; the diagonal 1-6 is interior
    faces += [[1, 6, 12], [6, 12, 13]]                       # a fin on it (edge 1-6 in three faces) and a face that keeps the fin attached
    faces += [[14, 15, 16], [16, 15, 14], [14, 15, 17], [15, 17, 18]]     # edge 14-15 three times: the first two share 15-16 and 16-14
    return np.asarray(faces, np.int64)


def main():
    gg.install_harness()
    import lib.cage as cage
    import lib.segmentation as seg
    import utils.mesh_utils as mu

    rng = np.random.default_rng(2024)
    meshes = {"grid": grid_mesh(6, 5), "octa": octahedron(2), "fins": fins_mesh()}
    out = {"names": np.array(list(meshes)), "sizes": np.asarray(SIZES), "rings": np.asarray(RINGS)}
    for name, faces in meshes.items():
        F = len(faces)
        pairs = mr.adjacency_pairs(faces)
        table = mr.neighbours_from_pairs(pairs, F)
        degree = (table >= 0).sum(1)
        assert degree.min() >= 1, "the reference's median raises on a face without neighbours"
        mesh = SimpleNamespace(faces=faces, face_adjacency=pairs)
        out[f"{name}_faces"], out[f"{name}_adjacency"] = faces.astype(np.int32), pairs.astype(np.int32)

        labels = rng.integers(0, 5, F)
        out[f"{name}_labels"] = labels.astype(np.int32)
        out[f"{name}_median"] = np.asarray(mu.median_filter_mesh(mesh, labels)).astype(np.int32)

        part = rng.integers(0, 5, (F, 9))
        part[rng.random((F, 9)) < 0.3] = 0
        part[0], part[1], part[2] = 0, [3, 1, 3, 1, 0, 0, 0, 0, 0], [4, 4, 2, 2, 0, 0, 0, 0, 0]      # no vote; two ties
        out[f"{name}_part_per_face"] = part.astype(np.int32)
        out[f"{name}_majority"] = np.asarray(seg.Segmenter.majority_vote(None, part)).astype(np.int32)

        masks = np.stack([rng.random(F) < 0.15, rng.random(F) < 0.5, np.arange(F) == F // 2, np.arange(F) < 3])
        out[f"{name}_masks"] = masks
        for n in RINGS:
            out[f"{name}_grown{n}"] = np.stack([cage.CageBase.grow_mask_region(None, mesh, m, n) for m in masks]).astype(bool)

        for H, W in SIZES:
            p2f, image = mr.random_fragments(int(rng.integers(1 << 30)), 1, H, W, F, 5)
            p2f = np.minimum(p2f, F - 1)                     # the reference indexes with every value >= 0
            assert (p2f == -1).any() and image.min() == 0 and image.max() == 4
            fragments = SimpleNamespace(pix_to_face=torch.from_numpy(p2f.astype(np.int64))[..., None])
            fake = SimpleNamespace(rasterizer=lambda meshes, cameras=None: fragments)
            colors = seg.Renderer.forward(fake, None, torch.zeros(1, 3, 3), torch.from_numpy(faces)[None], torch.from_numpy(image)[:, None])
            colors = colors.numpy()
            assert colors.shape == (F, 3) and (colors == colors[:, :1]).all()
            out[f"{name}_{H}x{W}_pix_to_face"], out[f"{name}_{H}x{W}_image"] = p2f[0], image[0].astype(np.uint8)
            out[f"{name}_{H}x{W}_part"] = colors[:, 0].astype(np.int32)
        print(name, "F", F, "degrees", np.bincount(degree, minlength=4).tolist())
    assert (mr.neighbours_from_pairs(out["fins_adjacency"], len(meshes["fins"]))[14] == 15).sum() == 2      # the doubled pair
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT))


if __name__ == "__main__":
    main()
