"""Gaussian initialisation without a GPU: the g++ build of csrc/gauss_init_math.h -- the text the kernels run -- against the oracle
(tests/gauss_init_ref.py), bit for bit; the oracle against the reference's own `sample_initial_points`
(tests/golden/gauss_init_cases.npz, tools/gen_gauss_init_golden.py); the fixed cases of every rule; the Python layer's ValueErrors;
`body_surface_draws` against the draws the reference made; the ABI surface and its refusals."""
import ctypes
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gauss_init_ref as gr
from conftest import ROOT

E_NULL, E_SIZE, E_CONFIG, E_CAPACITY = -1, -2, -3, -4        # D3GA_E_* (include/d3ga.h)
OUTPUTS = ("points", "rotations", "faces", "face_id", "barys")
CASES = ("body", "face", "upper", "solo")


def _same(a, b):
    for k in OUTPUTS:
        assert gr.same_bits(a[k], b[k]), k
    assert a["status"] == b["status"]


def _both(v, f, u, mask=None):
    """through the g++ build AND the oracle (they must agree bit for bit) -> the g++ build's dict with cum and k"""
    want, got = gr.sample(v, f, u, mask), gr.host_sample(v, f, u, mask, want_weights=True)
    _same(want, got)
    areas = gr.face_areas(v, f, mask)
    assert got["cum"] == gr.weights(areas)[1] and got["k"] == gr.shift(areas)
    return got


@pytest.mark.parametrize("F", [1, 2, 255, 256, 257, 513, 3000])
def test_host_build_equals_the_oracle(F):
    v, f = gr.random_mesh(F, F)
    mask = np.random.default_rng(F).random(F) < 0.5
    mask[F // 2] = True
    for n, m in ((1, None), (65, mask), (1000, None), (333, mask)):
        got = _both(v, f, gr.uniforms(n, 7 * F + n), m)
        assert got["status"] == 0 and got["cum"][-1] < 2 ** 62 and got["cum"][-1] >= 2 ** (61 - max(F - 1, 0).bit_length())
        if m is not None:
            assert mask[got["face_id"]].all()
        assert np.array_equal(f[got["face_id"]], got["faces"])
    normals, inflated = gr.host_normals(v, f, 0.03)
    want, condition = gr.vertex_normals_angle(v, f, want_condition=True)
    # acos is the one library call of the rules (Python's here, libm's there); everything else is the same float64 arithmetic
    assert (np.abs(normals - want).max(1) <= gr.normals_bound(condition)).all()
    assert gr.same_bits(inflated, v + 0.03 * normals)
    used = np.zeros(len(v), bool)
    used[f.reshape(-1)] = True
    assert np.allclose(np.linalg.norm(normals[used], axis=1), 1.0, atol=1e-12) and not normals[~used].any()


def test_oracle_equals_the_reference(golden):
    """face_id and faces equal; every float within one float32 unit in the last place of the array's largest magnitude: one rounding
    of float64 values whose own error (the order of a few float64 additions) is far below that unit.  Measured: the worst
    difference is 0 in all four cases (points, rotations and barys alike)."""
    z = golden("gauss_init_cases.npz")
    assert tuple(str(n) for n in z["names"]) == CASES
    v, f = z["vertices"], z["faces"]
    assert v.dtype == np.float64 and f.shape == (512, 3)
    worst = {}
    for tag in CASES:
        amount = float(z[f"{tag}_inflate"])
        mv = v + amount * gr.vertex_normals_angle(v, f) if amount else v
        parts, at = [], 0
        for mask, count in zip(z[f"{tag}_masks"], z[f"{tag}_counts"]):
            parts.append(gr.sample(mv, f, z[f"{tag}_uniforms"][at:at + count], mask))
            at += count
        got = {k: np.concatenate([p[k] for p in parts]) for k in OUTPUTS}
        assert all(p["status"] == 0 for p in parts) and at == len(z[f"{tag}_points"])
        assert np.array_equal(got["face_id"], z[f"{tag}_face_id"]) and np.array_equal(got["faces"], z[f"{tag}_faces"])
        for k in ("points", "rotations", "barys"):
            want = z[f"{tag}_{k}"]
            diff = float(np.abs(got[k].astype(np.float64) - want.astype(np.float64)).max())
            worst[(tag, k)] = diff
            print(f"{tag} {k}: worst difference {diff:.3e}, bound {gr.ulp32_of_largest(want):.3e}")
            assert diff <= gr.ulp32_of_largest(want), (tag, k, diff)
    assert float(z["upper_inflate"]) == 0.03 and int(z["body_discarded"]) == 2 and z["body_counts"].tolist() == [300, 700]


def test_fixed_cases_of_the_face_choice():
    tri = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
    # one triangle: every sample lands in it
    got = _both(tri, [[0, 1, 2]], gr.uniforms(50, 1))
    assert not got["face_id"].any() and (got["barys"] >= -1e-6).all() and np.allclose(got["barys"].sum(1), 1, atol=1e-6)
    # three faces of areas 0.5, 2, 0.5: u0 = 0 is the first face, u0 = 1 - 2^-53 the last
    v = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [0, 2, 0], [0, 0, 1]])
    f = np.array([[0, 1, 2], [0, 3, 4], [0, 1, 5]])
    u = np.array([[0.0, 0.2, 0.2], [1 - 2.0 ** -53, 0.2, 0.2], [0.5, 0.2, 0.2]])
    got = _both(v, f, u)
    assert got["face_id"].tolist() == [0, 2, 1]
    assert got["cum"] == [2 ** 57, 5 * 2 ** 57, 6 * 2 ** 57] and got["k"] == 58                     # max area 2 < 2^2, ceil(log2 3) = 2
    # a kept zero-area face between two others is never chosen, on a grid that hits every boundary region
    f0 = np.array([[0, 1, 2], [0, 1, 3], [0, 3, 4]])                                           # the middle one is collinear
    M = 4096
    grid = np.stack([(np.arange(M) + 0.5) / M, np.full(M, 0.3), np.full(M, 0.3)], 1)
    edge = np.array([[x, 0.1, 0.1] for x in (0.0, 0.2 - 2.0 ** -54, 0.2, 0.2 + 2.0 ** -54, 1 - 2.0 ** -53)])
    got = _both(v, f0, np.concatenate([grid, edge]))
    assert got["cum"][0] == got["cum"][1] and set(got["face_id"].tolist()) == {0, 2}
    # areas 0.5 and 2: the boundary is at 1/5.  The double 0.2 is 2^-55 above it, but m = floor(u0 2^53) is not: still face 0
    assert got["face_id"][M:].tolist() == [0, 0, 0, 2, 2]
    # a mask keeping one face; face_id still indexes the original list
    got = _both(v, f, gr.uniforms(40, 3), np.array([False, False, True]))
    assert (got["face_id"] == 2).all() and got["cum"][:2] == [0, 0]
    # leading and trailing faces of weight 0 at u0 = 0 and u0 = 1 - 2^-53
    got = _both(v, f, u, np.array([False, True, False]))
    assert got["face_id"].tolist() == [1, 1, 1]


def test_a_face_far_below_the_largest_gets_weight_zero():
    """The quantum is 2^-(62 - ceil(log2 F)) of 2^E: with F = 4097 (13 bits) a face 2^-50 of a largest face of area 0.5 2^E has
    weight floor(2^-2) = 0, and one of 2^-48 has weight 1."""
    F = 4097
    v = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [2.0 ** -25, 0, 0], [0, 2.0 ** -25, 0], [2.0 ** -24, 0, 0], [0, 2.0 ** -24, 0]])
    f = np.tile(np.array([[0, 1, 2]]), (F, 1))
    f[1], f[2] = [0, 3, 4], [0, 5, 6]
    areas = gr.face_areas(v, f)
    assert areas[1] == areas[0] * 2.0 ** -50 and areas[2] == areas[0] * 2.0 ** -48
    M = 8192
    grid = np.stack([(np.arange(M) + 0.5) / M, np.full(M, 0.3), np.full(M, 0.3)], 1)
    lead = np.array([[(1.0 / 4095) * (1 + j * 2.0 ** -38), 0.3, 0.3] for j in range(-8, 9)])      # around the end of face 0's share
    got = _both(v, f, np.concatenate([grid, lead]))
    q = np.diff([0] + got["cum"])
    assert got["k"] == 62 - 0 - 13 and q[0] == 2 ** 48 and q[1] == 0 and q[2] == 1
    assert 1 not in got["face_id"] and not got["face_id"][M:M + 8].any() and 0 not in got["face_id"][M + 9:]
    # ... while the same face among two is far above the quantum
    q2 = np.diff([0] + _both(v, f[:2], grid[:8])["cum"])
    assert q2[1] == 2 ** 10


def test_fixed_cases_of_the_point_and_the_barycentrics():
    v = np.array([[1.0, 2, 3], [3, 2, 3], [1, 6, 3]])
    f = [[0, 1, 2]]
    u = np.array([[0.5, 0.25, 0.75], [0.5, 0.75, 0.75], [0.5, 0.0, 0.0], [0.5, 0.5, 0.5 + 2.0 ** -53], [0.5, 0.125, 0.25]])
    got = _both(v, f, u)
    # r1 + r2 = 1 exactly is not folded; 0.75 + 0.75 folds to (0.25, 0.25); a sum one bit above 1 folds
    assert got["points"].tolist() == [[1.5, 5, 3], [1.5, 3, 3], [1, 2, 3], [2, 4, 3], [1.25, 3, 3]]
    assert np.abs(got["barys"] - np.array([[0, .25, .75], [.5, .25, .25], [1, 0, 0], [0, .5, .5], [.625, .125, .25]])).max() < 1e-7
    # the barycentrics are those of the FLOAT32 point: with vertices that float32 cannot hold they differ from (1 - r1 - r2, r1, r2)
    w = v + 1e-9 * np.array([[1.0, 2, 3], [5, 7, 11], [13, 17, 19]])
    got = _both(w, f, u[-1:])
    p = got["points"][0].astype(np.float64)
    e0, e1, v2 = w[1] - w[0], w[2] - w[0], p - w[0]
    d00, d01, d11, d20, d21 = e0 @ e0, e0 @ e1, e1 @ e1, v2 @ e0, v2 @ e1
    den = d00 * d11 - d01 * d01 + 1e-10
    assert np.allclose(got["barys"][0, 1:], [(d11 * d20 - d01 * d21) / den, (d00 * d21 - d01 * d20) / den], rtol=0, atol=1e-7)


def test_the_four_quaternion_branches():
    """One face per branch of matrix_to_quaternion's argmax, with a margin; the frame's B column is e0 x T = -|e0|^2 N, as the
    reference computes it."""
    rng = np.random.default_rng(5)
    found = {}
    for _ in range(10000):
        if len(found) == 4:
            break
        tri = rng.normal(size=(3, 3))
        _, _, _, T, B, N = gr.frames(tri, np.array([[0, 1, 2]]))
        q_abs = gr.quaternion_candidates(T, B, N)[0][0]
        order = np.argsort(q_abs)
        if q_abs[order[3]] - q_abs[order[2]] > 0.05:
            found.setdefault(int(order[3]), tri)
        assert np.allclose(B, -N, atol=1e-12)
    v = np.concatenate([found[b] for b in range(4)])
    f = np.arange(12).reshape(4, 3)
    mask = np.eye(4, dtype=bool)
    for b in range(4):
        got = _both(v, f, np.array([[0.5, 0.2, 0.3]]), mask[b])
        assert got["face_id"].tolist() == [b]
        _, _, _, T, B, N = gr.frames(v, f[b:b + 1])
        q_abs, cand = gr.quaternion_candidates(T, B, N)
        assert int(np.argmax(q_abs[0])) == b
        q = cand[0, b] * (1 if cand[0, b, 0] >= 0 else -1)
        assert np.array_equal(got["rotations"][0], q.astype(np.float32)) and got["rotations"][0, 0] >= 0
    import compat_ref as cr
    _, _, _, T, B, N = gr.frames(v, f)
    with cr.compat_path():
        from pytorch3d.transforms import matrix_to_quaternion
        want = matrix_to_quaternion(torch.from_numpy(np.stack([T, B, N], 2))).float().numpy()
    got = np.concatenate([gr.host_sample(v, f, np.array([[0.5, 0.2, 0.3]]), mask[b])["rotations"] for b in range(4)])
    assert np.abs(got - want).max() <= gr.ulp32_of_largest(want)


def test_nothing_to_sample_from_sets_the_status():
    v, f = gr.random_mesh(300, 2)
    u = gr.uniforms(10, 2)
    for mask, verts in ((np.zeros(300, bool), v), (None, np.zeros_like(v)), (None, np.tile(v[:1], (len(v), 1)))):
        got = _both(verts, f, u, mask)
        assert got["status"] == gr.STATUS_EMPTY and (got["face_id"] == -1).all()
        assert not got["points"].any() and not got["rotations"].any() and not got["barys"].any() and not got["faces"].any()
    # sticky: a later clean call leaves the bit set; a face naming a vertex outside the mesh weighs nothing and is flagged
    assert gr.host_sample(v, f, u, status=gr.STATUS_EMPTY)["status"] == gr.STATUS_EMPTY
    bad = f.copy()
    bad[7] = [0, 1, len(v)]
    bad[8] = [-1, 1, 2]
    got = gr.host_sample(v, bad, gr.uniforms(2000, 4), want_weights=True)
    assert got["status"] == gr.STATUS_RANGE and 7 not in got["face_id"] and 8 not in got["face_id"]
    assert got["cum"][7] == got["cum"][6] and got["cum"][8] == got["cum"][6]
    # areas that are not finite weigh nothing
    inf = v.copy()
    inf[f[3, 0]] = np.inf
    got = gr.host_sample(inf, f, gr.uniforms(500, 5), want_weights=True)
    touched = (f == f[3, 0]).any(1)
    assert got["status"] == 0 and not touched[got["face_id"]].any() and np.isfinite(got["points"]).all()


@pytest.mark.parametrize("F", [3, 257, 1000])
def test_counts_on_a_grid_equal_the_integer_oracle(F):
    v, f = gr.random_mesh(F, 100 + F)
    M = 20000
    u = np.stack([(np.arange(M) + 0.5) / M, np.full(M, 0.25), np.full(M, 0.5)], 1)
    got = gr.host_sample(v, f, u)
    _, cum = gr.weights(gr.face_areas(v, f))
    want = np.bincount([gr.pick_face(cum, x) for x in u[:, 0]], minlength=F)
    assert np.array_equal(np.bincount(got["face_id"], minlength=F), want)
    # and the counts follow the areas: within one sample per boundary of M area / sum(area)
    share = M * gr.face_areas(v, f) / gr.face_areas(v, f).sum()
    assert np.abs(want - share).max() <= 2.0


def _configs():
    four = {"body": dict(label_id=[-1], n_gaussians=700, n_under_gaussians=300), "face": dict(label_id=[-1], n_gaussians=150),
            "upper": dict(label_id=[1], n_gaussians=500, inflate=0.03), "lower": dict(label_id=[2], n_gaussians=500, inflate=0.03)}
    return four, {"body": dict(label_id=[-1], n_gaussians=400)}


def test_body_surface_draws_equal_the_reference(golden):
    from d3ga_amd.gauss_init import body_surface_draws
    z = golden("gauss_init_cases.npz")
    four, one = _configs()
    labels, region = z["face_to_label"], z["face_region"]
    assert z["body_cages"].tolist() == list(four) and z["body_label_ids"].tolist() == [-1, -1, 1, 2] and int(z["body_n_under"]) == 300
    assert z["body_n_gaussians"].tolist() == [700, 150, 500, 500] and z["solo_cages"].tolist() == ["body"]
    as_objects = {k: SimpleNamespace(**c) for k, c in four.items()}
    for tag, cages, name, face_mask in (("body", four, "body", region), ("face", four, "face", region), ("solo", one, "body", None),
                                        ("body", as_objects, "body", torch.from_numpy(region))):
        draws = body_surface_draws(torch.from_numpy(labels) if cages is as_objects else labels, cages, name, face_mask)
        assert [c for _, c in draws] == z[f"{tag}_counts"].tolist()
        for (mask, _), want in zip(draws, z[f"{tag}_masks"]):
            assert mask.dtype == bool and np.array_equal(mask, want)
    assert np.array_equal(z["body_masks"][0], ~region) and np.array_equal(z["body_masks"][1], (labels == 0) & ~region)
    assert np.array_equal(z["face_masks"][0], region) and np.array_equal(z["solo_masks"][0], np.ones(512, bool))
    # without a face cage the body keeps the face region, and the under-garment draw covers everything
    three = {k: c for k, c in four.items() if k != "face"}
    draws = body_surface_draws(labels, three, "body", region)
    assert draws[0][0].all() and np.array_equal(draws[1][0], labels == 0)
    bad = [lambda: body_surface_draws(labels, four, "upper"), lambda: body_surface_draws(labels, one, "face"),
           lambda: body_surface_draws(labels.astype(np.float32), four, "body"), lambda: body_surface_draws(labels[None], four, "body"),
           lambda: body_surface_draws(labels, four, "body", region[:-1]), lambda: body_surface_draws(labels, four, "body", labels),
           lambda: body_surface_draws(labels, {"body": dict(label_id=[-1])}, "body"),
           lambda: body_surface_draws(labels, {**four, "body": dict(label_id=[-1], n_gaussians=5, n_under_gaussians=0)}, "body")]
    for i, fn in enumerate(bad):
        with pytest.raises(ValueError):
            fn()
            pytest.fail(f"case {i} was accepted")


def test_python_layer_validates_on_the_host():
    from d3ga_amd import _lib
    from d3ga_amd.gauss_init import (SurfaceSamples, inflate, init_cage_parameters, sample_initial_points, sample_surface,
                                     vertex_normals_angle)
    vn, fn_ = gr.random_mesh(20, 1)
    v, f = torch.from_numpy(vn), torch.from_numpy(fn_)
    n = 8
    u = torch.rand(n, 3, dtype=torch.float64)
    out = SurfaceSamples.empty(16, "cpu")
    assert len(out) == 16 and len(out.rows(4, 12)) == n and out.rows(4, 12).status is out.status
    assert out.rows(4, 12).rotations.data_ptr() == out.rotations.data_ptr() + 64
    four, _ = _configs()
    config = SimpleNamespace(cages=four)
    labels = np.zeros(20, np.int64)
    body = dict(four["body"], cage_name="body")
    bad = [
        lambda: sample_surface(v, f, 0), lambda: sample_surface(v, f, -3), lambda: sample_surface(v, f, 2.5), lambda: sample_surface(v, f, True),
        lambda: sample_surface(v, f, 2 ** 29),
        lambda: sample_surface(v[:, :2], f, n), lambda: sample_surface(v.half(), f, n), lambda: sample_surface(v.long(), f, n),
        lambda: sample_surface(v[:0], f, n), lambda: sample_surface("mesh", f, n), lambda: sample_surface(v, "faces", n),
        lambda: sample_surface(v, f[:, :2], n), lambda: sample_surface(v, f.double(), n), lambda: sample_surface(v, f[:0], n),
        lambda: sample_surface(v, f.to(torch.int16), n),
        lambda: sample_surface(v, torch.zeros((2 ** 24, 3), dtype=torch.int32, device="meta"), n),
        lambda: sample_surface(v.to("meta"), f, n),                                            # faces and vertices on different devices
        lambda: sample_surface(v, f + len(v) - int(f.max()), n), lambda: sample_surface(v, f - 1 - int(f.min()), n),      # a vertex outside the mesh
        lambda: sample_surface(v, f, n, face_mask=torch.ones(19, dtype=torch.bool)), lambda: sample_surface(v, f, n, face_mask=torch.ones(20)),
        lambda: sample_surface(v, f, n, face_mask=torch.ones(20, 1, dtype=torch.bool)), lambda: sample_surface(v, f, n, face_mask=[1] * 20),
        lambda: sample_surface(v, f, n, face_mask=torch.ones(20, dtype=torch.bool, device="meta")),
        lambda: sample_surface(v, f, n, uniforms=u.float()), lambda: sample_surface(v, f, n, uniforms=u[:-1]), lambda: sample_surface(v, f, n, uniforms=u[:, :2]),
        lambda: sample_surface(v, f, n, uniforms=u, seed=3), lambda: sample_surface(v, f, n, uniforms=u.to("meta")),
        lambda: sample_surface(v, f, n, seed=1.5), lambda: sample_surface(v, f, n, seed="a"),
        lambda: sample_surface(v, f, n, block=96), lambda: sample_surface(v, f, n, block=2048),
        lambda: sample_surface(v, f, n, out=out), lambda: sample_surface(v, f, n, out=out.points), lambda: sample_surface(v, f, n, out=tuple(out)[:4]),
        lambda: sample_surface(v, f, n, out=SurfaceSamples(out.points[:n].double(), out.rotations[:n], out.faces[:n], out.face_id[:n], out.barys[:n], out.status)),
        lambda: sample_surface(v, f, n, out=SurfaceSamples(out.points[::2], out.rotations[:n], out.faces[:n], out.face_id[:n], out.barys[:n], out.status)),
        lambda: sample_surface(v, f, n, out=SurfaceSamples(out.points[:n], out.rotations[:n], out.faces[:n].long(), out.face_id[:n], out.barys[:n], out.status)),
        lambda: sample_surface(v, f, n, out=SurfaceSamples(out.points[:n], out.rotations[:n], out.faces[:n], out.face_id[:n], out.barys[:n], out.status.float())),
        lambda: sample_surface(v, f, n, out=SurfaceSamples.empty(n, "meta")),
        lambda: SurfaceSamples.empty(0, "cpu"), lambda: out.rows(4, 4), lambda: out.rows(-1, 4), lambda: out.rows(0, 17),
        lambda: inflate(v, f, float("nan")), lambda: inflate(v, f, float("inf")), lambda: inflate(v[:, :2], f, 0.1), lambda: inflate(v, f + 100, 0.1),
        lambda: vertex_normals_angle(v, f[:, :2]),
        lambda: sample_initial_points(v, f, dict(n_gaussians=5), config, labels), lambda: sample_initial_points(v, f, body, config),
        lambda: sample_initial_points(v, f, body, SimpleNamespace(), labels), lambda: sample_initial_points(v, f, body, config, labels[:-1]),
        lambda: sample_initial_points(v, f, body, config, labels, uniforms=torch.rand(999, 3, dtype=torch.float64)),
        lambda: sample_initial_points(v, f, body, config, labels, uniforms=torch.rand(1000, 3)),
        lambda: sample_initial_points(v, f, body, config, labels, uniforms=torch.rand(1000, 3, dtype=torch.float64), seed=1),
        lambda: sample_initial_points(v, f, dict(cage_name="upper", inflate=0.03), config), lambda: sample_initial_points(v, f, dict(cage_name="upper", n_gaussians=0), config),
        lambda: init_cage_parameters(out.points[:3], out.rotations[:3], 8, 3), lambda: init_cage_parameters(out.points.double(), out.rotations, 8, 3),
        lambda: init_cage_parameters(out.points, out.rotations[:8], 8, 3), lambda: init_cage_parameters(out.points, out.points, 8, 3),
        lambda: init_cage_parameters(out.points, out.rotations, 0, 3), lambda: init_cage_parameters(out.points, out.rotations, 8, 4),
        lambda: init_cage_parameters(out.points, out.rotations, 8, -1), lambda: init_cage_parameters(out.points, out.rotations, 8, 3, generator=7),
        lambda: init_cage_parameters(out.points.numpy(), out.rotations, 8, 3), lambda: init_cage_parameters(out.points, out.rotations.to("meta"), 8, 3),
    ]
    for i, fn in enumerate(bad):
        with pytest.raises(ValueError):
            fn()
            pytest.fail(f"case {i} was accepted")
    # everything fits, but the tensors live on the CPU: no fallback, and nothing was launched
    ok = [lambda: sample_surface(v, f, n), lambda: sample_surface(v.float(), f.int(), n, uniforms=u, face_mask=torch.ones(20, dtype=torch.bool)),
          lambda: sample_surface(v, f, n, seed=3, out=out.rows(8, 16), block=64), lambda: sample_surface(v, f, n, out=tuple(out.rows(0, 8))),
          lambda: inflate(v, f, 0.1), lambda: vertex_normals_angle(v[None], f[None]),
          lambda: sample_initial_points(v, f, body, config, labels, seed=1),
          lambda: sample_initial_points(v, f, dict(four["upper"], cage_name="upper"), config, seed=1),
          lambda: init_cage_parameters(out.points, out.rotations, 8, 3, generator=torch.Generator())]
    for fn in ok:
        with pytest.raises(_lib.D3GAError):
            fn()
    if not torch.cuda.is_available():
        with pytest.raises(_lib.D3GAError):
            sample_surface(vn, fn_, n)                       # arrays are uploaded: without a GPU that is the package's usual error
    for bit in (_lib.SAMPLE_STATUS_EMPTY, _lib.SAMPLE_STATUS_RANGE):
        out.status[0] = bit
        with pytest.raises(ValueError):
            out.check()
    out.status[0] = 0
    assert out.check() is out


def test_new_abi_surface():
    from d3ga_amd import _lib
    src = open(os.path.join(ROOT, "include", "d3ga.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], capture_output=True, text=True, check=True).stdout
    for name, n_args in (("d3ga_surface_sample_scratch_bytes", 2), ("d3ga_surface_sample", 17), ("d3ga_vertex_normals_angle", 11)):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
        assert re.search(r"\bT %s$" % name, out, flags=re.M)                     # through csrc/d3ga.map
        assert len(_lib._SIGNATURES[name][0]) == n_args
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, src).group(1)
        assert decl.count(",") + 1 == n_args
    assert _lib.ABI_VERSION == 112 and re.search(r"#define\s+D3GA_VERSION\s+112\b", src) and _lib.lib().d3ga_version() == 112
    for name, value in (("SAMPLE_MAX_FACES", gr.MAX_FACES), ("SAMPLE_STATUS_EMPTY", gr.STATUS_EMPTY), ("SAMPLE_STATUS_RANGE", gr.STATUS_RANGE)):
        assert getattr(_lib, name) == value and re.search(r"#define\s+D3GA_%s\s+%d\b" % (name, value), src), name
    build = open(os.path.join(ROOT, "d3ga_amd", "csrc", "build.py")).read()
    assert "gauss_init.hip" in build and "gauss_init_math.h" in build and 'EXTRA["gauss_init.hip"] = ["-ffp-contract=off"]' in build
    import d3ga_amd
    from d3ga_amd import gauss_init
    for name in gauss_init.__all__:
        assert name in d3ga_amd.__all__ and getattr(d3ga_amd, name) is getattr(gauss_init, name)
    n = ctypes.c_int64(-1)
    L = _lib.lib()
    for F in (1, 255, 256, 257, 65537, 2 ** 24 - 1):
        assert L.d3ga_surface_sample_scratch_bytes(F, ctypes.byref(n)) == 0 and n.value == gr.lib().hc_surface_sample_scratch_bytes(F)
        blocks = (F + 255) // 256
        assert n.value % 256 == 0 and n.value >= 256 + 8 * F + 8 * blocks + 8 * (blocks + 1)
    assert L.d3ga_surface_sample_scratch_bytes(0, ctypes.byref(n)) == E_SIZE and L.d3ga_surface_sample_scratch_bytes(2 ** 24, ctypes.byref(n)) == E_SIZE
    assert L.d3ga_surface_sample_scratch_bytes(5, None) == E_NULL


@pytest.mark.parametrize("which", ["library", "host build"])
def test_entry_points_refuse_bad_arguments_before_any_launch(which):
    """The refusals happen before any HIP call: host buffers stand in for device memory and are never touched.  The g++ build runs
    the same check functions and must give the same statuses."""
    from d3ga_amd import _lib
    buf = (ctypes.c_uint8 * 8192)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) & ~255)
    at = lambda k: ctypes.c_void_p(p.value + k)
    ok = dict(V=4, F=2, n=3, verts=p, faces=p, face_mask=None, uniforms=p, points=p, rotations=p, out_faces=p, face_id=p, barys=p, scratch=p,
              scratch_bytes=1024, status=p, block=0)
    if which == "library":
        sample = lambda **kw: _lib.lib().d3ga_surface_sample(*{**ok, **kw}.values(), None)
        normals = lambda *a: _lib.lib().d3ga_vertex_normals_angle(*a, None)
    else:
        sample = lambda **kw: gr.lib().hc_surface_sample(*{**ok, **kw}.values())
        normals = gr.lib().hc_vertex_normals_angle
    for name in ("V", "F", "n"):
        assert sample(**{name: 0}) == E_SIZE and sample(**{name: -1}) == E_SIZE, name
    assert sample(F=2 ** 24, scratch_bytes=2 ** 40) == E_SIZE and sample(V=2 ** 30) == E_SIZE and sample(n=2 ** 29) == E_SIZE
    assert sample(block=96) == E_CONFIG and sample(block=-64) == E_CONFIG and sample(block=2048) == E_CONFIG
    for name in ("verts", "faces", "uniforms", "points", "rotations", "out_faces", "face_id", "barys", "scratch", "status"):
        assert sample(**{name: None}) == E_NULL, name
        assert sample(**{name: at(1)}) == E_CONFIG, name
    assert sample(verts=at(4)) == E_CONFIG and sample(uniforms=at(4)) == E_CONFIG and sample(scratch=at(128)) == E_CONFIG
    assert sample(scratch_bytes=1023) == E_CAPACITY and sample(F=257, scratch_bytes=256 + 2304 + 256 + 255) == E_CAPACITY
    q, r, s = at(1024), at(2048), at(3072)
    assert normals(0, 2, p, p, p, p, 0.1, q, r, s) == E_SIZE and normals(4, 0, p, p, p, p, 0.1, q, r, s) == E_SIZE
    assert normals(4, 2 ** 24, p, p, p, p, 0.1, q, r, s) == E_SIZE
    assert normals(4, 2, p, p, p, p, float("nan"), q, r, s) == E_CONFIG and normals(4, 2, p, p, p, p, float("inf"), q, r, s) == E_CONFIG
    for k in range(4):
        a = [p, p, p, p]
        a[k] = None
        assert normals(4, 2, *a, 0.1, q, r, s) == E_NULL
        a[k] = at(1)
        assert normals(4, 2, *a, 0.1, q, r, s) == E_CONFIG
    assert normals(4, 2, p, p, p, p, 0.1, None, None, s) == E_NULL and normals(4, 2, p, p, p, p, 0.1, q, r, None) == E_NULL
    assert normals(4, 2, p, p, p, p, 0.1, at(1028), r, s) == E_CONFIG and normals(4, 2, p, p, p, p, 0.1, q, at(2052), s) == E_CONFIG
    assert normals(4, 2, p, p, p, p, 0.1, p, r, s) == E_CONFIG and normals(4, 2, p, p, p, p, 0.1, q, p, s) == E_CONFIG      # in place
    assert not any(buf)
