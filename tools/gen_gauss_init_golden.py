#!/usr/bin/env python3
"""Generate tests/golden/gauss_init_cases.npz -- and nothing else -- by running the reference's OWN functions on the CPU:

    lib.cage.CageBase.sample_initial_points(self)      with sample_body_surface, grow_mask_region, get_face_mask and
    lib.cage.CageBase.compute_tris_bary(self, ...)     compute_tris_bary as they are, on a CageBase whose attributes are set here

Runs only where the reference checkout is present; no test runs it.  The import-stub harness is tools/gen_golden.py's
`install_harness`.  Two of its stubs get content here, so parity with trimesh and pytorch3d stays UNPINNED:

    trimesh   a mesh object with the attributes lib/cage.py touches.  `sample.sample_surface` follows trimesh's documented steps --
              searchsorted(cumsum(area_faces), u0 sum(area_faces)); lengths (u1, u2), folded by |l - 1| where their sum exceeds 1;
              origin + sum(lengths * edge vectors) -- on uniforms drawn HERE and recorded, not on numpy's global stream.
              `vertex_normals` follows rule 6 of csrc/gauss_init_math.h (tests/gauss_init_ref.py::vertex_normals_angle);
              `face_adjacency` is tests/mesh_labels_ref.py::adjacency_pairs.
    pytorch3d `matrix_to_quaternion` is compat/pytorch3d/transforms.py.

The generator asserts its own conditions, so that the reference alone decides every case: every u0 sum(area) lies at least
1e-9 sum(area) from a cumulative boundary, no r1 + r2 lies within 1e-9 of 1 (rows that would are redrawn before the reference
sees them), and the winning candidate of the quaternion rule leads the runner-up by at least 1e-6.

Arrays only.  One closed mesh (a subdivided octahedron, stretched and jittered, 512 faces) with part labels 0 / 1 / 2 and a face
region.  Cases: `body` of a four-cage avatar (under-garment draw + outside-garment draw, no face region), `face` of the same,
`upper` of the same (inflated by 0.03), `solo` = the body cage of a one-cage avatar.  Per case: the draws the reference KEPT, in
the order it concatenates them (mask over the original faces, count, uniforms), the number of draws it made and threw away, and
what it returned: points, rotations, faces, barys, plus the original index of every sample's face."""
import importlib.util
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
import mesh_labels_ref as mr  # noqa: E402

OUT = os.path.join(HERE, "..", "tests", "golden", "gauss_init_cases.npz")


class Cfg(dict):
    """a mapping with attribute access, as the reference's OmegaConf nodes"""
    __getattr__ = dict.__getitem__


def octahedron(levels):
    verts = [(1.0, 0, 0), (-1.0, 0, 0), (0, 1.0, 0), (0, -1.0, 0), (0, 0, 1.0), (0, 0, -1.0)]
    faces = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    for _ in range(levels):
        mid, out = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                mid[key] = len(verts)
                p = (np.asarray(verts[a]) + np.asarray(verts[b])) / 2
                verts.append(tuple(p / np.linalg.norm(p)))
            return mid[key]
        for a, b, c in faces:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            out += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        faces = out
    return np.asarray(verts, np.float64), np.asarray(faces, np.int64)


class StubMesh:
    def __init__(self, vertices, faces, face_index=None):
        self.vertices, self.faces = np.array(vertices, np.float64), np.array(faces, np.int64)
        self.face_index = np.arange(len(self.faces)) if face_index is None else np.array(face_index)

    def copy(self):
        return StubMesh(self.vertices, self.faces, self.face_index)

    def update_faces(self, mask):
        mask = np.asarray(mask, bool)
        self.faces, self.face_index = self.faces[mask], self.face_index[mask]

    @property
    def face_adjacency(self):
        return mr.adjacency_pairs(self.faces)

    @property
    def vertex_normals(self):
        return gr.vertex_normals_angle(self.vertices, self.faces)

    @property
    def area_faces(self):
        return gr.face_areas(self.vertices, self.faces)


class Sampler:
    """trimesh.sample.sample_surface on recorded uniforms"""

    def __init__(self, seed, n_faces):
        self.rng, self.F, self.calls = np.random.default_rng(seed), n_faces, []

    def sample_surface(self, mesh, count):
        count = int(count)
        area = mesh.area_faces
        total, cum = area.sum(), np.cumsum(area)
        u = self.rng.random((count, 3))
        for _ in range(100):                                 # the generator's conditions: redraw the rows that sit on a decision
            near = np.abs(cum[None, :] - (u[:, 0] * total)[:, None]).min(1) < 1e-9 * total
            near |= np.abs(u[:, 1] + u[:, 2] - 1.0) < 1e-9
            if not near.any():
                break
            u[near] = self.rng.random((int(near.sum()), 3))
        assert not near.any()
        index = np.searchsorted(cum, u[:, 0] * total)
        origins = mesh.vertices[mesh.faces[index, 0]]
        vectors = np.stack([mesh.vertices[mesh.faces[index, 1]] - origins, mesh.vertices[mesh.faces[index, 2]] - origins], 1)
        lengths = u[:, 1:3].copy()
        fold = lengths.sum(1) > 1.0
        lengths[fold] -= 1.0
        lengths = np.abs(lengths)
        samples = (vectors * lengths[:, :, None]).sum(1) + origins
        mask = np.zeros(self.F, bool)
        mask[mesh.face_index] = True
        self.calls.append(dict(mask=mask, count=count, uniforms=u, samples=samples, face_id=mesh.face_index[index]))
        return samples, index


def compat_matrix_to_quaternion():
    spec = importlib.util.spec_from_file_location("_d3ga_compat_transforms", os.path.join(HERE, "..", "compat", "pytorch3d", "transforms.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.matrix_to_quaternion


def kept_draws(calls, points):
    """the calls whose samples the reference returned, in the order it concatenated them"""
    order, at = [], 0
    left = list(range(len(calls)))
    while at < len(points):
        hit = [i for i in left if at + calls[i]["count"] <= len(points) and
               np.array_equal(calls[i]["samples"].astype(np.float32), points[at:at + calls[i]["count"]])]
        assert len(hit) == 1, (at, hit)
        order.append(hit[0])
        left.remove(hit[0])
        at += calls[hit[0]]["count"]
    return order, len(left)


def main():
    gg.install_harness()
    import lib.cage as cage
    cage.matrix_to_quaternion = compat_matrix_to_quaternion()

    verts, faces = octahedron(3)
    rng = np.random.default_rng(2025)
    verts = verts * np.array([0.35, 0.9, 0.25]) + rng.normal(size=verts.shape) * 0.004
    F = len(faces)
    height = verts[faces].mean(1)[:, 1]
    labels = np.where((height > 0.1) & (height < 0.55), 1, np.where((height < -0.05) & (height > -0.7), 2, 0)).astype(np.int64)
    region = height > 0.7
    colors = np.zeros((F, 4), np.uint8)
    colors[region, 0] = 255
    assert region.sum() > 8 and (labels == 1).sum() > 50 and (labels == 2).sum() > 50 and (labels == 0).sum() > 50

    four = Cfg(body=Cfg(label_id=[-1], inflate=0.01, n_gaussians=700, n_under_gaussians=300), face=Cfg(label_id=[-1], inflate=0.0, n_gaussians=150),
               upper=Cfg(label_id=[1], inflate=0.03, n_gaussians=500), lower=Cfg(label_id=[2], inflate=0.03, n_gaussians=500))
    one = Cfg(body=Cfg(label_id=[-1], inflate=0.01, n_gaussians=400))
    cases = {"body": (four, "body", True), "face": (four, "face", True), "upper": (four, "upper", True), "solo": (one, "body", False)}

    out = {"names": np.array(list(cases)), "vertices": verts, "faces": faces.astype(np.int32), "face_to_label": labels.astype(np.int32),
           "face_region": region}
    worst_margin = np.inf
    for seed, (tag, (cages, name, with_region)) in enumerate(cases.items()):
        sampler = Sampler(100 + seed, F)
        cage.trimesh = SimpleNamespace(sample=SimpleNamespace(sample_surface=sampler.sample_surface))
        geo = cage.CageBase()
        geo.config = Cfg(cages=cages)
        geo.cage_config = Cfg(cages[name], cage_name=name)
        geo.inflate_cage = cages[name]["inflate"]
        geo.mc_source = StubMesh(verts, faces)
        geo.face_to_label = labels
        geo.face_mask = SimpleNamespace(visual=SimpleNamespace(face_colors=colors)) if with_region else None
        points, rots, tri, barys = geo.sample_initial_points()
        assert points.dtype == torch.float32 and rots.dtype == torch.float32 and tri.dtype == torch.int32 and barys.dtype == torch.float32
        points, rots, tri, barys = points.numpy(), rots.numpy(), tri.numpy(), barys.numpy()
        order, discarded = kept_draws(sampler.calls, points)
        kept = [sampler.calls[i] for i in order]
        amount = 0.0 if name in ("body", "face") else float(cages[name]["inflate"])
        face_id = np.concatenate([c["face_id"] for c in kept])
        assert np.array_equal(faces[face_id], tri)
        # compute_tris_bary once more, called directly
        mv = verts + amount * gr.vertex_normals_angle(verts, faces)
        v0, v1, v2 = (torch.from_numpy(mv[tri[:, c]]) for c in range(3))
        again = cage.CageBase.compute_tris_bary(None, torch.from_numpy(points).double(), v0, v1, v2).float().numpy()
        assert np.array_equal(again, barys)
        _, _, _, T, B, N = gr.frames(mv, tri.astype(np.int64))
        q_abs = np.sort(gr.quaternion_candidates(T, B, N)[0], 1)
        worst_margin = min(worst_margin, float((q_abs[:, 3] - q_abs[:, 2]).min()))
        out[f"{tag}_name"] = np.array(name)
        out[f"{tag}_cages"] = np.array(list(cages))
        out[f"{tag}_label_ids"] = np.array([cages[k]["label_id"][0] for k in cages], np.int32)
        out[f"{tag}_n_gaussians"] = np.array([cages[k]["n_gaussians"] for k in cages], np.int32)
        out[f"{tag}_n_under"] = np.array(cages[name].get("n_under_gaussians", 0), np.int32)
        out[f"{tag}_with_region"] = np.array(with_region)
        out[f"{tag}_inflate"] = np.array(amount)
        out[f"{tag}_masks"] = np.stack([c["mask"] for c in kept])
        out[f"{tag}_counts"] = np.array([c["count"] for c in kept], np.int32)
        out[f"{tag}_uniforms"] = np.concatenate([c["uniforms"] for c in kept])
        out[f"{tag}_discarded"] = np.array(discarded, np.int32)
        out[f"{tag}_points"], out[f"{tag}_rotations"], out[f"{tag}_faces"], out[f"{tag}_barys"] = points, rots, tri, barys
        out[f"{tag}_face_id"] = face_id.astype(np.int32)
        print(tag, "draws kept", [c["count"] for c in kept], "discarded", discarded, "points", points.shape)
    assert worst_margin >= 1e-6, worst_margin
    print("quaternion margin", worst_margin)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT))


if __name__ == "__main__":
    main()
