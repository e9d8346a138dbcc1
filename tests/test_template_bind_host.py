"""Template binding without a GPU: the g++ build of csrc/template_bind_math.h -- the text the kernels run -- against the oracle
(tests/template_bind_ref.py), bit for bit; the oracle against the reference's own `subdivide_loop`, `Smplman.find_nn` and
`Smplman.unpose` (tests/golden/template_bind_cases.npz, tools/gen_template_bind_golden.py); the fixed cases of every rule; the Python
layer's ValueErrors; the ABI surface and its refusals."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import template_bind_ref as tr
from conftest import ROOT

E_NULL, E_SIZE, E_CONFIG, E_CAPACITY = -1, -2, -3, -4        # D3GA_E_* (include/d3ga.h)
GOLDEN_MESHES = ("sphere", "grid", "quad")
ENTRY_POINTS = (("d3ga_loop_edge_keys", 6), ("d3ga_loop_plan_scratch_bytes", 3), ("d3ga_loop_plan_build", 8), ("d3ga_loop_subdivide", 8),
                ("d3ga_loop_faces", 4), ("d3ga_unpose", 15))


def _both(v, f, a, iterations=1):
    """through the g++ build AND the oracle (they must agree bit for bit) -> the oracle's triple"""
    want, got = tr.subdivide(v, f, a, iterations), tr.host_subdivide(v, f, a, iterations)
    for x, y in zip(want, got):
        assert (x is None and y is None) or tr.same_bits(x, y)
    return want


def _meshes(V):
    if V >= 255:
        yield tr.bipyramid(V - 2, seed=V)
        yield tr.open_mesh(V, seed=V)
        if V == 255:
            yield tr.torus(15, 17, seed=V)
        if V == 256:
            yield tr.torus(16, 16, seed=V)
    if V >= 3000:
        yield tr.torus(50, 60, seed=V)
        yield tr.grid(55, 55, seed=V)


@pytest.mark.parametrize("V", [1, 2, 255, 256, 257, 3000])
def test_host_build_equals_the_oracle(V):
    """Closed and open meshes with face rows permuted and corners rotated at random.  V = 1 and V = 2 admit no face of three distinct
    vertices: the plan is flagged, holds no edge, and both say so the same way; unpose runs at n = V for every size."""
    rng = np.random.default_rng(V)
    if V < 3:
        f = np.zeros((2, 3), np.int32) if V == 1 else np.array([[0, 1, 0], [1, 0, 5]], np.int32)
        p, h = tr.plan(f, V), tr.host_plan(f, V)
        tr.same_plan(p, h)
        assert p["E"] == 0 and p["status"] == (tr.STATUS_DEGENERATE if V == 1 else tr.STATUS_DEGENERATE | tr.STATUS_RANGE)
    for v, f in _meshes(V):
        v, f = tr.shuffled(v, f, V)
        p, h = tr.plan(f, len(v)), tr.host_plan(f, len(v))
        tr.same_plan(p, h)
        assert p["status"] == 0 and p["E"] == len(np.unique(np.sort(np.stack([f, np.roll(f, -1, 1)], -1).reshape(-1, 2), 1), axis=0))
        nv, nf, na = _both(v.astype(np.float32), f, tr.attributes(len(v), 5, seed=V))
        assert nv.shape == (len(v) + p["E"], 3) and nf.shape == (4 * len(f), 3) and na.shape == (len(v) + p["E"], 5)
        assert np.isfinite(nv).all() and np.allclose(na[len(v):].sum(1), 1, atol=1e-5)       # the odd stencils' coefficients sum to 1
        _both(v, f.astype(np.int64), None)                   # float64 vertices, int64 faces, no attributes
    # unpose: dense float32 and float64 tables and the sparse form, with rows and offsets
    n, J, R = V, 9, 40
    A, w = tr.rigid_transforms(J, seed=V), tr.attributes(R, J, seed=V)
    q, rows, bs = rng.normal(size=(n, 3)), rng.integers(0, R, n), rng.normal(size=(R, 3)) * 0.01
    want, status = tr.unpose(q, A, w, rows, bs)
    assert status == 0 and np.isfinite(want).all()
    for skin in (w, w.astype(np.float64)):
        got, st = tr.host_unpose(q, A, skin, rows, bs)
        assert st == 0 and tr.same_bits(want, got)
    order = np.argsort(w == 0, axis=1, kind="stable")[:, :int((w != 0).sum(1).max())]       # non-zero weights first, in joint order
    assert (np.take_along_axis(w, order, 1) != 0).sum() == (w != 0).sum()
    sparse = (order.astype(np.int32), np.take_along_axis(w, order, 1))
    for fn in (tr.unpose, tr.host_unpose):
        got, st = fn(q, A, sparse, rows, bs)
        assert st == 0 and tr.same_bits(want, got)
    assert np.abs(want - tr.unpose_f64(q, A, w, rows, bs)).max() <= 2.0 ** -24 * np.abs(want).max() + 1e-12


def _golden_case(z, tag):
    return {k[len(tag) + 1:]: z[k] for k in z.files if k.startswith(tag + "_")}


def test_oracle_equals_the_reference_ids(golden):
    """Faces and nearest ids are exactly the reference's.  The dense query leaves out the odd vertices of boundary edges: they are
    the midpoints of their edges, equidistant from both ends by construction (the generator asserts that these are the only ties)."""
    z = golden("template_bind_cases.npz")
    assert tuple(str(n) for n in z["names"]) == GOLDEN_MESHES
    for tag in GOLDEN_MESHES:
        c = _golden_case(z, tag)
        v, f = c["vertices"], c["faces"]
        assert v.dtype == np.float32 and c["weights"].dtype == np.float32 and c["sub_vertices"].dtype == np.float64
        nv, nf, _ = tr.subdivide(v, f, c["weights"])
        assert np.array_equal(nf, c["sub_faces"]) and nf.dtype == c["sub_faces"].dtype
        rows = c["dense_rows"]
        assert np.array_equal(tr.nearest(v, c["sub_vertices"])[rows], c["dense_ids"][rows])
        assert np.array_equal(tr.nearest(tr.inflate(v, f, float(c["inflate"])), c["cage"]), c["cage_ids"])
        p = tr.plan(f, len(v))
        left_out = np.setdiff1d(np.arange(len(nv)), rows)
        assert np.array_equal(left_out, len(v) + np.nonzero(p["edge_boundary"])[0])
    assert len(_golden_case(z, "sphere")["dense_rows"]) == 66 + 192 and float(z["sphere_inflate"]) == 0.02


def test_oracle_equals_the_reference_stencils(golden):
    """Even rows within 2^-24 max|x| of the reference's float64 values (one rounding); odd rows within 8 x 2^-24 max|x| (the reference
    evaluates them in float32: seven float32 operations with coefficients summing to 1, plus our one rounding).
    Measured worst differences, in units of 2^-24 max|x| (positions / weights): sphere even 0.50 / 0.66, odd 2.01 / 1.44;
    grid even 0.78 / 0.72, odd 0.89 / 0.96; quad even 0.00 / 0.46, odd 0.00 / 0.00."""
    z = golden("template_bind_cases.npz")
    for tag in GOLDEN_MESHES:
        c = _golden_case(z, tag)
        V = len(c["vertices"])
        nv, _, nw = tr.subdivide(c["vertices"], c["faces"], c["weights"])
        for name, ours, ref in (("positions", nv, c["sub_vertices"]), ("weights", nw, c["sub_weights"])):
            unit = 2.0 ** -24 * np.abs(ref).max()
            even = np.abs(ours[:V].astype(np.float64) - ref[:V]).max() / unit
            odd = np.abs(ours[V:].astype(np.float64) - ref[V:]).max() / unit
            print(f"{tag} {name}: even {even:.2f}, odd {odd:.2f} (units of 2^-24 max|x|)")
            assert even <= 1.0 and odd <= 8.0, (tag, name, even, odd)
    # the quirk is the reference's: the quad's diagonal ends have three boundary neighbours and their weights sum to 9/8
    q = _golden_case(z, "quad")
    assert np.allclose(q["sub_weights"][[0, 2]].sum(1), 1.125, atol=1e-6) and np.allclose(q["sub_weights"][[1, 3]].sum(1), 1.0, atol=1e-6)


def test_oracle_equals_the_reference_unpose(golden):
    """The reference inverts a float32 4x4 in float32, so no bound can be derived for it.  Its own error against the float64 value is
    formed from the golden, element by element, and ours may differ from it by that error plus our one rounding.
    Measured: the reference's worst error is 2.2e-07 (sphere), 6.2e-07 (grid), 1.2e-07 (quad); ours against the float64 value is
    5.9e-08, 2.3e-07 and 4.5e-08, below one rounding (2^-24 max|x|: 7.9e-08, 2.8e-07, 6.7e-08) throughout."""
    z = golden("template_bind_cases.npz")
    for tag in GOLDEN_MESHES:
        c = _golden_case(z, tag)
        nv, skin = c["sub_vertices"].astype(np.float32), c["sub_weights"].astype(np.float32)       # what the reference fed
        ours, status = tr.unpose(nv, c["joint_mats"], skin, c["dense_ids"], c["blend_offsets"])
        exact = tr.unpose_f64(nv, c["joint_mats"], skin, c["dense_ids"], c["blend_offsets"])
        ref = c["unposed"].astype(np.float64)
        ref_err = np.abs(ref - exact)
        rounding = 2.0 ** -24 * np.abs(exact).max()
        print(f"{tag}: reference error {ref_err.max():.2e}, ours {np.abs(ours - exact).max():.2e}, one rounding {rounding:.2e}")
        assert status == 0 and c["unposed"].dtype == np.float32
        assert (np.abs(ours.astype(np.float64) - ref) <= ref_err + rounding).all()


def test_fixed_cases():
    # a tetrahedron: every valence 3, beta_3 = 3/16: even = (7/16) v + (3/16) (the other three); centroid kept
    v, f = tr.tetrahedron()
    nv, nf, na = _both(v, f, np.eye(4))
    b3 = tr.beta_table(3)[3]
    assert abs(b3 - 3 / 16) < 1e-15 and nv.shape == (10, 3) and nf.shape == (16, 3)
    assert np.allclose(nv[:4], (1 - 3 * b3) * v + b3 * (v.sum(0) - v), atol=1e-7) and np.allclose(na[:4], 7 / 16 * np.eye(4) + 3 / 16 * (1 - np.eye(4)))
    p = tr.plan(f, 4)
    assert p["edge_verts"].tolist() == [[0, 1], [0, 2], [1, 2], [0, 3], [1, 3], [2, 3]] and not p["edge_boundary"].any()
    assert np.allclose(na[4], [0.375, 0.375, 0.125, 0.125]) and np.allclose(na[4:].sum(1), 1)
    # a single triangle: every edge a boundary edge, odd = midpoints, even = 3/4 v + 1/8 (the other two)
    v, f = tr.triangle()
    nv, nf, _ = _both(v, f, None)
    assert np.allclose(nv[:3], 0.75 * v + (v.sum(0) - v) / 8, atol=1e-7) and np.allclose(nv[3:], [(v[0] + v[1]) / 2, (v[0] + v[2]) / 2, (v[1] + v[2]) / 2], atol=1e-7)
    assert nf.tolist() == [[0, 3, 4], [3, 1, 5], [4, 5, 2], [3, 5, 4]]
    # the quad: the diagonal 0-2 is interior, yet its ends are boundary vertices with THREE boundary neighbours: weights sum to 9/8
    v, f = tr.quad()
    nv, nf, na = _both(v, f, np.ones((4, 1)))
    assert na[:4, 0].tolist() == [1.125, 1.0, 1.125, 1.0] and (na[4:] == 1).all()
    assert np.allclose(nv[0], 0.75 * v[0] + (v[1] + v[2] + v[3]) / 8, atol=1e-7) and np.allclose(nv[1], 0.75 * v[1] + (v[0] + v[2]) / 8, atol=1e-7)
    p = tr.plan(f, 4)
    assert p["edge_verts"].tolist() == [[0, 1], [0, 2], [1, 2], [0, 3], [2, 3]] and p["edge_boundary"].tolist() == [1, 0, 1, 1, 1]
    assert p["edge_opp"][1].tolist() == [1, 3] and p["edge_faces"][1].tolist() == [0, 1]                 # x2: the face of lower index
    assert np.allclose(nv[5], 0.375 * (v[0] + v[2]) + (v[1] + v[3]) / 8, atol=1e-7)
    # an unreferenced vertex is kept, with its attributes
    v, f = tr.tetrahedron()
    v5, a5 = np.concatenate([v, [[9.0, 8, 7]]]), np.arange(10.0).reshape(5, 2)
    nv, nf, na = _both(v5, f, a5)
    assert nv[4].tolist() == [9, 8, 7] and na[4].tolist() == [8, 9] and tr.same_bits(nv[:4], tr.subdivide(v, f)[0][:4]) and nf.min() == 0 and (nf != 4).all()
    # an edge in three faces
    fan = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int32)
    p, h = tr.plan(fan, 5), tr.host_plan(fan, 5)
    tr.same_plan(p, h)
    assert p["status"] == tr.STATUS_NONMANIFOLD and p["edge_faces"][0].tolist() == [0, 1]
    for fn in (tr.subdivide, tr.host_subdivide):
        with pytest.raises(ValueError, match="shared by more than 2 faces"):
            fn(np.zeros((5, 3)), fan)
    # two disjoint tetrahedra: the parts do not see each other
    v, f = tr.tetrahedron()
    v2, f2 = np.concatenate([v, v * 0.5 + 7]), np.concatenate([f, f + 4])
    nv, nf, _ = _both(v2, f2, None)
    one, other = tr.subdivide(v, f)[0], tr.subdivide(v * 0.5 + 7, f)[0]
    assert tr.same_bits(nv[:4], one[:4]) and tr.same_bits(nv[4:8], other[:4]) and tr.same_bits(nv[8:14], one[4:]) and tr.same_bits(nv[14:], other[4:])
    # iterations = 2 is two calls
    v, f = tr.grid(4, 3)
    a = tr.attributes(12, 3)
    twice = _both(v, f, a, iterations=2)
    once = tr.subdivide(v, f, a)
    for x, y in zip(twice, tr.subdivide(*once)):
        assert tr.same_bits(x, y)
    assert twice[1].shape == (16 * len(f), 3)
    # the unique edges do not depend on the order of the face rows, nor on the corner a face starts with: same rows, same bits
    v, f = tr.grid(17, 17, seed=2)
    v, a = v.astype(np.float32), tr.attributes(len(v), 7, seed=9)
    first, moved = tr.subdivide(v, f, a), tr.subdivide(v, tr.shuffled(v, f, 5)[1], a)
    assert tr.same_bits(first[0], moved[0]) and tr.same_bits(first[2], moved[2]) and not np.array_equal(first[1], moved[1])


def test_fixed_cases_of_unpose():
    q = np.array([[1.0, 2, 3], [-1, 0.5, 2]])
    eye = np.eye(4)[None]
    for fn in (tr.unpose, tr.host_unpose):
        # one joint, the identity: v - bs
        got, st = fn(q, eye, np.ones((2, 1), np.float32), None, np.array([[0.5, 0, 0], [0, 0.25, 0]]))
        assert st == 0 and got.tolist() == [[0.5, 2, 3], [-1, 0.25, 2]]
        # a rotation by 90 degrees about z with a translation, weight 2: s = 2 scales the translation back
        A = np.array([[[0.0, -1, 0, 3], [1, 0, 0, 4], [0, 0, 1, 5], [0, 0, 0, 1]]])
        got, st = fn(q[:1], A, np.full((1, 1), 2.0), None, None)
        assert st == 0 and np.allclose(got, [[(2 - 4) / 2, -(1 - 3) / 2, (3 - 5) / 2]])
        # two opposite rotations about z, half and half: M has a zero 2x2 block -- singular, flagged, zeros and no NaN
        half = np.stack([A[0], np.array([[0.0, 1, 0, 0], [-1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])])
        got, st = fn(q, half, np.array([[0.5, 0.5], [1.0, 0.0]], np.float32), None, None)
        assert st == tr.STATUS_SINGULAR and got[0].tolist() == [0, 0, 0] and np.isfinite(got).all() and got[1].any()
        # weights that cancel: s = 0
        got, st = fn(q[:1], np.concatenate([eye, 2 * eye]), np.array([[1.0, -1.0]]), None, None)
        assert st == tr.STATUS_SINGULAR and not got.any()
        # a row or a joint outside its table
        got, st = fn(q, eye, np.ones((2, 1), np.float32), np.array([0, 2]), None)
        assert st == tr.STATUS_RANGE and got[1].tolist() == [0, 0, 0] and got[0].tolist() == [1, 2, 3]
        got, st = fn(q, eye, (np.array([[0, 1], [0, 0]], np.int32), np.array([[1.0, 0.5], [1.0, 0.0]], np.float32)), None, None)
        assert st == tr.STATUS_RANGE and got.tolist() == q.tolist()


def test_python_layer_refuses_bad_input():
    from d3ga_amd import _lib, template_bind as tb
    v, f = (torch.from_numpy(x) for x in tr.grid(4, 3))
    a = torch.rand(12, 5)
    A, w, rows, bs = torch.eye(4)[None].repeat(3, 1, 1), torch.rand(12, 3), torch.zeros(12, dtype=torch.int64), torch.zeros(12, 3)
    nan_v = v.clone()
    nan_v[3, 1] = float("nan")
    bad = [
        lambda: tb.loop_plan(f.float(), 12), lambda: tb.loop_plan(f[:, :2], 12), lambda: tb.loop_plan(f[:0], 12), lambda: tb.loop_plan(f, 0),
        lambda: tb.loop_plan(f, 12.0), lambda: tb.loop_plan(f, True), lambda: tb.loop_plan([[0, 1, 2]], 3),
        lambda: tb.loop_subdivide(v, f, iterations=0), lambda: tb.loop_subdivide(v, f, iterations=1.5), lambda: tb.loop_subdivide(v[:, :2], f),
        lambda: tb.loop_subdivide(v.half(), f), lambda: tb.loop_subdivide(v, f, a[:-1]), lambda: tb.loop_subdivide(v, f, a.long()),
        lambda: tb.loop_subdivide(v, f, a[:, 0]), lambda: tb.loop_subdivide(v, f, plan="plan"), lambda: tb.loop_subdivide("v", f),
        lambda: tb.loop_subdivide(v, f.to("meta")), lambda: tb.loop_subdivide(v, f, a.to("meta")),
        lambda: tb.nearest_vertex(v[:, :2], f, v), lambda: tb.nearest_vertex(v, f, v[:, :2]), lambda: tb.nearest_vertex(v, f, v, float("nan")),
        lambda: tb.nearest_vertex(v, f, v, float("inf")), lambda: tb.nearest_vertex(v, f, v.to("meta")), lambda: tb.nearest_vertex(v.long(), f, v),
        lambda: tb.unpose(v[:, :2], A, w), lambda: tb.unpose(v, A[:, :3], w), lambda: tb.unpose(v, A.long(), w), lambda: tb.unpose(v, "A", w),
        lambda: tb.unpose(v, A, w[:, :2]), lambda: tb.unpose(v, A, w[:5]), lambda: tb.unpose(v, A, w, rows[:5]), lambda: tb.unpose(v, A, w, rows.float()),
        lambda: tb.unpose(v, A, w, rows, bs[:, :2]), lambda: tb.unpose(v, A, (rows, w)), lambda: tb.unpose(v, A, (w.long(), w, w)),
        lambda: tb.unpose(v, A, (w, w)), lambda: tb.unpose(v, A, w.to("meta")), lambda: tb.unpose(v, A, w, rows.to("meta")),
        lambda: tb.bind_cage(None, "binding", v, 0.0), lambda: tb.bind_cage_skin(v, f, v, 0.0, w, w[:5]), lambda: tb.bind_cage_skin(v, f, v, 0.0, w[0], w[0]),
        lambda: tb.bind_cage_skin(v, f, v, 0.0, w[:5], w[:5]),
    ]
    for i, fn in enumerate(bad):
        with pytest.raises(ValueError):
            fn()
            pytest.fail(f"case {i} was accepted")
    # everything fits, but the tensors live on the CPU: no fallback, and nothing was launched
    ok = [lambda: tb.loop_plan(f, 12), lambda: tb.loop_plan(f.long()[None], 12), lambda: tb.loop_subdivide(v, f), lambda: tb.loop_subdivide(v.float(), f.long(), a, iterations=2),
          lambda: tb.nearest_vertex(v, f, v, 0.1), lambda: tb.unpose(v, A, w), lambda: tb.unpose(v[None], A[None], (rows[:, None].int(), w[:, :1]), rows, bs[None]),
          lambda: tb.bind_cage_skin(v, f, v, 0.0, w, w.long())]
    for fn in ok:
        with pytest.raises(_lib.D3GAError):
            fn()
    if not torch.cuda.is_available():
        with pytest.raises(_lib.D3GAError):
            tb.loop_subdivide(v.numpy(), f.numpy())          # arrays are uploaded: without a GPU that is the package's usual error
    # what the status word turns into
    for bit, text in ((_lib.BIND_STATUS_NONMANIFOLD, "shared by more than 2 faces"), (_lib.BIND_STATUS_RANGE, "outside"),
                      (_lib.BIND_STATUS_DEGENERATE, "twice"), (_lib.BIND_STATUS_SINGULAR, "singular")):
        with pytest.raises(ValueError, match=text):
            tb.Unposed(v, torch.tensor([bit], dtype=torch.int32)).check()
    u = tb.Unposed(v, torch.zeros(1, dtype=torch.int32))
    assert u.check() is u and tuple(u)[0] is v
    assert tr.same_bits(tb.beta_table(70), tr.beta_table(70)) and tb.beta_table(3)[0] == 0


def test_new_abi_surface():
    from d3ga_amd import _lib
    src = open(os.path.join(ROOT, "include", "d3ga.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], capture_output=True, text=True, check=True).stdout
    for name, n_args in ENTRY_POINTS:
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
        assert re.search(r"\bT %s$" % name, out, flags=re.M)                     # through csrc/d3ga.map
        assert len(_lib._SIGNATURES[name][0]) == n_args
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, src).group(1)
        assert decl.count(",") + 1 == n_args
    assert _lib.ABI_VERSION == 112 and re.search(r"#define\s+D3GA_VERSION\s+112\b", src) and _lib.lib().d3ga_version() == 112
    for name, value in (("RANGE", tr.STATUS_RANGE), ("NONMANIFOLD", tr.STATUS_NONMANIFOLD), ("DEGENERATE", tr.STATUS_DEGENERATE),
                        ("SINGULAR", tr.STATUS_SINGULAR)):
        assert getattr(_lib, "BIND_STATUS_" + name) == value and re.search(r"#define\s+D3GA_BIND_STATUS_%s\s+%d\b" % (name, value), src), name
    assert _lib.LOOP_BAD_KEY == tr.BAD_KEY and re.search(r"#define\s+D3GA_LOOP_BAD_KEY\s+0x7fffffffffffffffLL", src)
    assert ctypes.sizeof(_lib.LoopPlanTables) == ctypes.sizeof(tr.PlanStruct) == 16 + 8 * 8
    assert [n for n, _ in _lib.LoopPlanTables._fields_] == [n for n, _ in tr.PlanStruct._fields_]
    build = open(os.path.join(ROOT, "d3ga_amd", "csrc", "build.py")).read()
    assert "template_bind.hip" in build and "template_bind_math.h" in build and 'EXTRA["template_bind.hip"] = ["-ffp-contract=off"]' in build
    import d3ga_amd
    from d3ga_amd import template_bind
    for name in template_bind.__all__:
        assert name in d3ga_amd.__all__ and getattr(d3ga_amd, name) is getattr(template_bind, name)
    n = ctypes.c_int64(-1)
    L = _lib.lib()
    for V, F in ((1, 1), (255, 500), (256, 86), (257, 65537), (10475, 20908), (5, 2 ** 28)):
        assert L.d3ga_loop_plan_scratch_bytes(V, F, ctypes.byref(n)) == 0 and n.value == tr.lib().hc_loop_plan_scratch_bytes(V, F)
        blocks = (max(3 * F, V) + 255) // 256
        assert n.value % 256 == 0 and n.value >= 12 * F + 4 * (3 * F + 1) + 8 * V + 4 * blocks + 8 * (blocks + 1)
    for V, F in ((0, 4), (4, 0), (-1, 4), (4, 2 ** 29)):
        assert L.d3ga_loop_plan_scratch_bytes(V, F, ctypes.byref(n)) == E_SIZE and tr.lib().hc_loop_plan_scratch_bytes(V, F) == E_SIZE
    assert L.d3ga_loop_plan_scratch_bytes(5, 5, None) == E_NULL


@pytest.mark.parametrize("which", ["library", "host build"])
def test_entry_points_refuse_bad_arguments_before_any_launch(which):
    """The refusals happen before any HIP call: host buffers stand in for device memory and are never touched.  The g++ build runs
    the same check functions and must give the same statuses."""
    from d3ga_amd import _lib
    buf = (ctypes.c_uint8 * 8192)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) & ~255)
    at = lambda k: ctypes.c_void_p(p.value + k)
    tables = dict.fromkeys(tr.PLAN_TABLES, p.value)
    if which == "library":
        L, S, tail = _lib.lib(), _lib.LoopPlanTables, (None,)
        keys, build, sub, faces, unpose = L.d3ga_loop_edge_keys, L.d3ga_loop_plan_build, L.d3ga_loop_subdivide, L.d3ga_loop_faces, L.d3ga_unpose
    else:
        L, S, tail = tr.lib(), tr.PlanStruct, ()
        keys, build, sub, faces, unpose = L.hc_loop_edge_keys, L.hc_loop_plan_build, L.hc_loop_subdivide, L.hc_loop_faces, L.hc_unpose
    plan = lambda **kw: ctypes.byref(S(**{**dict(V=4, F=2, E=5, reserved=0), **tables, **kw}))
    # keys
    assert keys(0, 2, p, p, p, *tail) == E_SIZE and keys(4, 0, p, p, p, *tail) == E_SIZE and keys(4, 2 ** 29, p, p, p, *tail) == E_SIZE
    for k in range(3):
        a = [p, p, p]
        a[k] = None
        assert keys(4, 2, *a, *tail) == E_NULL
        a[k] = at(1)
        assert keys(4, 2, *a, *tail) == E_CONFIG
    assert keys(4, 2, p, at(4), p, *tail) == E_CONFIG
    # build
    ok = [p, p, p, p, p, 4096]
    assert build(None, *ok, *tail) == E_NULL and build(plan(V=0), *ok, *tail) == E_SIZE and build(plan(F=-2), *ok, *tail) == E_SIZE
    for name in tr.PLAN_TABLES:
        assert build(plan(**{name: None}), *ok, *tail) == E_NULL, name
        if "boundary" not in name:
            assert build(plan(**{name: p.value + 2}), *ok, *tail) == E_CONFIG, name
    for k in range(5):
        a = list(ok)
        a[k] = None
        assert build(plan(), *a, *tail) == E_NULL
        a[k] = at(1)
        assert build(plan(), *a, *tail) == E_CONFIG
    assert build(plan(), p, at(4), p, p, p, 4096, *tail) == E_CONFIG and build(plan(), p, p, p, p, at(128), 4096, *tail) == E_CONFIG
    need = tr.lib().hc_loop_plan_scratch_bytes(4, 2)
    assert build(plan(), p, p, p, p, p, need - 1, *tail) == E_CAPACITY
    # subdivide and faces
    ok = [3, p, p, 8, p, p]
    assert sub(None, *ok, *tail) == E_NULL and sub(plan(E=0), *ok, *tail) == E_SIZE and sub(plan(E=7), *ok, *tail) == E_SIZE
    assert sub(plan(), 0, p, p, 8, p, p, *tail) == E_SIZE and sub(plan(), 3, p, p, 0, p, p, *tail) == E_SIZE
    assert sub(plan(vert_nbr=None), *ok, *tail) == E_NULL
    for k in (1, 2, 4, 5):
        a = list(ok)
        a[k] = None
        assert sub(plan(), *a, *tail) == E_NULL
        a[k] = at(1)
        assert sub(plan(), *a, *tail) == E_CONFIG
    assert sub(plan(), 3, at(4), p, 8, p, p, *tail) == E_CONFIG
    assert faces(None, p, p, *tail) == E_NULL and faces(plan(E=0), p, p, *tail) == E_SIZE and faces(plan(), None, p, *tail) == E_NULL
    assert faces(plan(), p, None, *tail) == E_NULL and faces(plan(), at(2), p, *tail) == E_CONFIG and faces(plan(face_edge=None), p, p, *tail) == E_NULL
    # unpose
    ok = dict(n=4, J=3, R=5, K=3, vertices=p, joint_mats=p, skin_w=p, w_f64=0, skin_idx=None, rows=None, offsets=None, n_offsets=0, out=p, status=p)
    call = lambda **kw: unpose(*{**ok, **kw}.values(), *tail)
    for name in ("n", "J", "R", "K"):
        assert call(**{name: 0}) == E_SIZE and call(**{name: -3}) == E_SIZE, name
    assert call(K=2) == E_SIZE and call(K=2, skin_idx=p, out=None) == E_NULL and call(R=2 ** 30, K=4, skin_idx=p) == E_SIZE and call(n=2 ** 30) == E_SIZE
    assert call(offsets=p, n_offsets=0) == E_SIZE
    for name in ("vertices", "joint_mats", "skin_w", "out", "status"):
        assert call(**{name: None}) == E_NULL, name
        assert call(**{name: at(1)}) == E_CONFIG, name
    assert call(w_f64=2) == E_CONFIG and call(w_f64=1, skin_w=at(4)) == E_CONFIG and call(skin_w=at(4), out=None) == E_NULL
    assert call(skin_idx=at(2)) == E_CONFIG and call(rows=at(4)) == E_CONFIG and call(offsets=at(4), n_offsets=5) == E_CONFIG and call(vertices=at(4)) == E_CONFIG
    assert not any(buf)
