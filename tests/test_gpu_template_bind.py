"""Template binding on the GPU (d3ga_amd/template_bind.py, csrc/template_bind.hip): the kernels against the oracle
(tests/template_bind_ref.py) bit for bit -- vertices, attributes, faces and every table of the plan; determinism; the status word;
nearest_vertex; unpose with its round trip through lbs_cage; and the reference's call shapes end to end on a synthetic SMPL-X
model.  The oracle itself is held to the g++ build of the header and to the reference in tests/test_template_bind_host.py."""
import numpy as np
import pytest
import torch

import template_bind_ref as tr

pytestmark = pytest.mark.gpu
DEV = "cuda"
_CACHE = {}


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def mesh(name):
    """the meshes the tests share, built once: (vertices float32, faces int32)"""
    if name not in _CACHE:
        v, f = {"tetrahedron": tr.tetrahedron, "triangle": tr.triangle, "quad": tr.quad, "grid17": lambda: tr.grid(17, 17, seed=2),
                "bipyramid70": lambda: tr.bipyramid(70, seed=2), "sphere128": lambda: tr.sphere(2, seed=3, jitter=0.03),
                "sphere8192": lambda: tr.sphere(5, seed=4, jitter=0.002)}[name]()
        _CACHE[name] = (v.astype(np.float32), f)
    return _CACHE[name]


def oracle_plan(name):
    key = ("plan", name)
    if key not in _CACHE:
        v, f = mesh(name)
        _CACHE[key] = tr.plan(f, len(v))
    return _CACHE[key]


def plan_tables(p):
    out = {k: host(getattr(p, k)) for k in tr.PLAN_TABLES}
    out.update(V=p.V, F=p.F, E=p.E, max_valence=p.max_valence, status=p.status)
    return out


@pytest.mark.parametrize("name,C", [("tetrahedron", 4), ("triangle", 2), ("quad", 1), ("grid17", 5), ("bipyramid70", 3), ("sphere128", 7),
                                    ("sphere8192", 55)])
def test_kernels_equal_the_oracle(name, C):
    from d3ga_amd import loop_plan, loop_subdivide
    v, f = mesh(name)
    a = tr.attributes(len(v), C, seed=1)
    p = oracle_plan(name)
    got = loop_plan(dev(f), len(v))
    tr.same_plan(p, plan_tables(got))
    assert got.check() is got and got.valence.cpu().tolist() == np.diff(p["vert_offsets"]).tolist()
    nv, nf, na = loop_subdivide(dev(v), dev(f), dev(a), plan=got)
    assert nv.dtype == torch.float32 and na.dtype == torch.float32 and nf.dtype == torch.int32
    assert tr.same_bits(host(nv), tr.stencil(p, v)) and tr.same_bits(host(na), tr.stencil(p, a))
    assert np.array_equal(host(nf), tr.new_faces(p)) and nf.shape == (4 * len(f), 3)
    if name in ("grid17", "bipyramid70"):
        assert p["max_valence"] == (8 if name == "grid17" else 70) and p["vert_boundary"].any() == (name == "grid17")


@pytest.mark.parametrize("C", [0, 1, 3, 4, 55, 58])
def test_attribute_widths(C):
    from d3ga_amd import loop_subdivide
    v, f = mesh("sphere128")
    a = tr.attributes(len(v), C, seed=C)
    nv, nf, na = loop_subdivide(dev(v), dev(f), dev(a))
    p = oracle_plan("sphere128")
    assert tuple(na.shape) == (len(v) + p["E"], C) and tr.same_bits(host(nv), tr.stencil(p, v))
    assert tr.same_bits(host(na), tr.stencil(p, a) if C else np.zeros((len(v) + p["E"], 0), np.float32))
    # float64 inputs: the same rule, no rounding on the way in
    a64 = a.astype(np.float64) + 1e-9
    got = loop_subdivide(dev(v.astype(np.float64)), dev(f), dev(a64))
    assert tr.same_bits(host(got[0]), tr.stencil(p, v)) and (C == 0 or tr.same_bits(host(got[2]), tr.stencil(p, a64)))


def test_determinism_and_two_levels():
    from d3ga_amd import loop_subdivide
    v, f = mesh("grid17")
    a = tr.attributes(len(v), 7, seed=9)
    first = loop_subdivide(dev(v), dev(f), dev(a))
    again = loop_subdivide(dev(v), dev(f), dev(a))
    wide = loop_subdivide(dev(v), dev(f).long(), dev(a))
    assert wide[1].dtype == torch.int64 and torch.equal(wide[1], first[1].long())
    for x, y, z in zip(first, again, wide):
        assert torch.equal(x, y) and torch.equal(x, z if z.dtype == x.dtype else z.to(x.dtype))
    # the unique edges do not depend on the order of the face rows (nor on which corner a face starts with): same rows, same bits
    _, fp = tr.shuffled(v, f, 5)
    moved = loop_subdivide(dev(v), dev(fp), dev(a))
    assert tr.same_bits(host(moved[0]), host(first[0])) and tr.same_bits(host(moved[2]), host(first[2]))
    assert not np.array_equal(host(moved[1]), host(first[1]))
    # iterations = 2 equals two calls, and the oracle
    twice = loop_subdivide(dev(v), dev(f), dev(a), iterations=2)
    step = loop_subdivide(*first)
    want = tr.subdivide(v, f, a, iterations=2)
    for x, y, w in zip(twice, step, want):
        assert torch.equal(x, y) and tr.same_bits(host(x), w)


def test_status():
    from d3ga_amd import _lib, loop_plan, loop_subdivide
    v = torch.zeros(5, 3, device=DEV)
    fan = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int32)
    p = loop_plan(dev(fan), 5)
    tr.same_plan(tr.plan(fan, 5), plan_tables(p))
    assert p.status == _lib.BIND_STATUS_NONMANIFOLD
    with pytest.raises(ValueError, match="shared by more than 2 faces"):
        p.check()
    with pytest.raises(ValueError, match="shared by more than 2 faces"):
        loop_subdivide(v, dev(fan))
    for bad, bit, text in ((np.array([[0, 1, 2], [2, 1, 5]], np.int32), _lib.BIND_STATUS_RANGE, "outside"),
                           (np.array([[0, 1, 2], [2, 1, -1]], np.int64), _lib.BIND_STATUS_RANGE, "outside"),
                           (np.array([[0, 1, 2], [2, 1, 2 ** 32 + 3]], np.int64), _lib.BIND_STATUS_RANGE, "outside"),
                           (np.array([[0, 1, 2], [2, 1, 1]], np.int32), _lib.BIND_STATUS_DEGENERATE, "twice")):
        p = loop_plan(dev(bad), 5)
        tr.same_plan(tr.plan(np.clip(bad, -1, 2 ** 31 - 1), 5), plan_tables(p))
        assert p.status == bit and p.E == 3 and host(p.face_edge)[1].tolist() == [-1, -1, -1]
        with pytest.raises(ValueError, match=text):
            loop_subdivide(v, dev(bad))
    with pytest.raises(ValueError, match="finite"):
        loop_subdivide(torch.full((5, 3), float("nan"), device=DEV), dev(fan[:1]))
    # a vertex no face names passes through with its attributes
    tv, tf = mesh("tetrahedron")
    v5, a5 = np.concatenate([tv, [[9.0, 8, 7]]]).astype(np.float32), np.arange(10, dtype=np.float32).reshape(5, 2)
    nv, nf, na = loop_subdivide(dev(v5), dev(tf), dev(a5))
    want = tr.subdivide(v5, tf, a5)
    assert host(nv)[4].tolist() == [9, 8, 7] and host(na)[4].tolist() == [8, 9]
    assert tr.same_bits(host(nv), want[0]) and tr.same_bits(host(na), want[2]) and np.array_equal(host(nf), want[1])


def test_nearest_vertex():
    from d3ga_amd import nearest_vertex
    # duplicate candidates: the lowest index; one candidate; 257 queries
    t = np.array([[0.0, 0, 0], [1, 0, 0], [1, 0, 0], [0, 1, 0], [1, 0, 0]], np.float32)
    f = np.array([[0, 1, 3]], np.int32)
    q = np.random.default_rng(0).normal(size=(257, 3)).astype(np.float32)
    q[:3] = [[1, 0, 0], [0.9, 0.1, 0], [2, -1, 0.5]]
    ids = nearest_vertex(dev(t), dev(f), dev(q))
    assert ids.dtype == torch.int64 and tuple(ids.shape) == (257,) and ids[:3].tolist() == [1, 1, 1]
    assert np.array_equal(host(ids), tr.nearest(t, q)) and 2 not in ids.tolist() and 4 not in ids.tolist()
    assert nearest_vertex(dev(t[:1]), dev(f), dev(q)).tolist() == [0] * 257
    assert nearest_vertex(dev(t), dev(f), dev(q[:1])).tolist() == [1]
    # an inflated against an uninflated template on the (stretched) sphere: the inflation moves the choice, as the oracle says.  The normals
    # call acos (host and device may differ in the last bits of a float64), so ids are held exactly where the float64 margin is
    # clear and to the smallest distance everywhere
    v, f = mesh("sphere128")
    v = (v * np.array([0.35, 0.9, 0.25])).astype(np.float32)             # stretched: the normals are not the radii
    rng = np.random.default_rng(4)
    q = (v[rng.integers(0, len(v), 400)] * 1.3 + rng.normal(size=(400, 3)) * 0.05).astype(np.float32)
    plain, puffed = host(nearest_vertex(dev(v), dev(f), dev(q))), host(nearest_vertex(dev(v), dev(f), dev(q), inflate=0.2))
    assert np.array_equal(plain, tr.nearest(v, q))
    moved = tr.inflate(v, f, 0.2)
    want, best, second = tr.nearest_margin(moved, q)
    clear = second - best > 1e-5 * second
    assert clear.sum() > 350 and np.array_equal(puffed[clear], want[clear])
    assert (((q.astype(np.float64) - moved[puffed]) ** 2).sum(1) <= best * (1 + 1e-5)).all()
    assert (plain != puffed).sum() > 10


@pytest.mark.parametrize("n", [1, 255, 257])
def test_unpose_equals_the_oracle_and_returns_through_lbs_cage(n):
    from d3ga_amd import unpose
    from d3ga_amd.cage_deform import lbs_cage, sparse_skin_weights
    rng = np.random.default_rng(n)
    J, R = 55, 300
    A = tr.rigid_transforms(J, seed=n, angle=0.6).astype(np.float32)
    w = tr.attributes(R, J, seed=n)
    q = rng.normal(size=(n, 3)).astype(np.float32)
    rows, bs = rng.integers(0, R, n), (rng.normal(size=(R, 3)) * 0.01).astype(np.float32)
    want, status = tr.unpose(q, A, w, rows, bs)
    assert status == 0
    dense = unpose(dev(q), dev(A), dev(w), dev(rows), dev(bs)).check()
    assert tr.same_bits(host(dense.vertices), want) and dense.status.item() == 0
    # the K-sparse table that holds the same weights: the same bits, whether indexed by rows or gathered first
    idx, sw = sparse_skin_weights(dev(w))
    assert torch.equal(unpose(dev(q)[None], dev(A)[None], (idx, sw), dev(rows).int(), dev(bs)[None]).check().vertices, dense.vertices)
    gi, gw = sparse_skin_weights(dev(w), rows=dev(rows))
    gathered = unpose(dev(q), dev(A).double(), (gi, gw.double()), None, None).check().vertices
    assert tr.same_bits(host(gathered), tr.unpose(q, A, (host(gi), host(gw)), None, None)[0])
    # round trip: posing the unposed vertices again returns the input, within the tolerance of lbs_cage's own forward tests
    back = lbs_cage(dense.vertices, dev(bs)[dev(rows)], dev(A), gi, gw)
    np.testing.assert_allclose(host(back), q, rtol=1e-5, atol=1e-5 * float(np.abs(q).max()))


def test_unpose_fixed_cases():
    from d3ga_amd import _lib, unpose
    q = np.array([[1.0, 2, 3], [-1, 0.5, 2]], np.float32)
    eye = torch.eye(4, device=DEV)[None]
    bs = np.array([[0.5, 0, 0], [0, 0.25, 0]], np.float32)
    got = unpose(dev(q), eye, torch.ones(2, 1, device=DEV), None, dev(bs)).check()
    assert host(got.vertices).tolist() == (q - bs).tolist()
    # two opposite rotations about z, half and half: singular, flagged, and no NaN comes back
    half = dev(np.array([[[0.0, -1, 0, 3], [1, 0, 0, 4], [0, 0, 1, 5], [0, 0, 0, 1]], [[0.0, 1, 0, 0], [-1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]], np.float32))
    w = np.array([[0.5, 0.5], [1.0, 0.0]], np.float32)
    got = unpose(dev(q), half, dev(w))
    vertices, status = got
    assert status.item() == _lib.BIND_STATUS_SINGULAR and torch.isfinite(vertices).all() and vertices[0].tolist() == [0, 0, 0]
    assert tr.same_bits(host(vertices), tr.unpose(q, host(half), w)[0])
    with pytest.raises(ValueError, match="singular"):
        got.check()
    # a row outside the table
    got = unpose(dev(q), eye, torch.ones(2, 1, device=DEV), dev(np.array([0, 7])))
    assert got.status.item() == _lib.BIND_STATUS_RANGE and host(got.vertices).tolist() == [[1, 2, 3], [0, 0, 0]]
    with pytest.raises(ValueError, match="outside"):
        got.check()
    with pytest.raises(ValueError, match="finite"):
        unpose(dev(q), eye * float("inf"), torch.ones(2, 1, device=DEV))


@pytest.fixture(scope="module")
def layer(tmp_path_factory):
    """a synthetic SMPL-X model over the closed 512-face sphere: 55 joints, random skinning, the sphere's faces"""
    import d3ga_amd.synthetic as syn
    from d3ga_amd.body_model import SMPLlayer
    v, f = tr.sphere(3, seed=6, jitter=0.005)
    data = syn.smpl_model_data("smplx", seed=3, V=len(v))
    data["f"] = f.astype(np.int64)
    data["v_template"] = v * np.array([0.3, 0.8, 0.25])
    d = tmp_path_factory.mktemp("template_bind_model")
    syn.write_smpl_model(str(d / "SMPLX_NEUTRAL.pkl"), data)
    return SMPLlayer(str(d), model_type="smplx", gender="neutral", use_joints=True, regressor_path=None).to(DEV)


def test_bind_body_template_and_cage_end_to_end(layer):
    from d3ga_amd import TemplateBinding, bind_body_template, bind_cage, star_pose
    from d3ga_amd.cage_deform import lbs_cage, sparse_skin_weights
    verts, T, A, bs = star_pose(layer)
    V, J = layer.V, layer.J
    assert tuple(verts.shape) == (1, V, 3) and tuple(A.shape) == (1, J, 4, 4) and tuple(bs.shape) == (1, V, 3)
    poses = torch.zeros(1, layer.NUM_POSES, device=DEV)
    poses[:, 5], poses[:, 8] = np.pi / 6, -np.pi / 6
    zero = torch.zeros(1, 3, device=DEV)
    again = layer(poses=poses, shapes=torch.zeros(1, 10, device=DEV), Rh=zero, Th=zero, expression=torch.zeros(1, 10, device=DEV))
    assert all(torch.equal(x, y) for x, y in zip((verts, T, A, bs), again))
    v, f, w = host(verts[0]), host(layer.faces_tensor), host(layer.weights)
    off = (np.random.default_rng(8).normal(size=(V, 3)) * 0.002).astype(np.float32)
    for offset, densify in ((None, True), (off, True), (None, False)):
        b = bind_body_template(layer, inflate=0.0, densify=densify, offset=None if offset is None else dev(offset))
        assert isinstance(b, TemplateBinding)
        base = v if offset is None else (v.astype(np.float64) + offset).astype(np.float32)
        nv, nf, nw = tr.subdivide(base, f, w) if densify else (base, f, w)
        ids = tr.nearest(base, nv)
        vtn, status = tr.unpose(nv, host(A[0]), nw, ids, host(bs[0]))
        assert status == 0 and np.array_equal(host(b.nn_ids), ids) and b.nn_ids.dtype == torch.int64
        assert np.array_equal(host(b.body_template_faces), nf) and b.body_template_faces.dtype == layer.faces_tensor.dtype
        assert tr.same_bits(host(b.skin_weights), nw) and tr.same_bits(host(b.body_template_vertices), vtn[None])
    # the cage: points off the surface, bound to the ORIGINAL template inflated by 0.01, skinned by the even rows of the dense table
    b = bind_body_template(layer)
    rng = np.random.default_rng(12)
    cage = (v[rng.integers(0, V, 700)] * 1.1 + rng.normal(size=(700, 3)) * 0.01).astype(np.float32)
    c = bind_cage(layer, b, dev(cage), 0.01)
    want, best, second = tr.nearest_margin(tr.inflate(v, f, 0.01), cage)
    clear = second - best > 1e-5 * second
    ids = host(c.nn_ids)
    assert clear.sum() > 600 and np.array_equal(ids[clear], want[clear]) and ids.max() < V
    vtn, status = tr.unpose(cage, host(A[0]), host(b.skin_weights), ids, host(bs[0]))
    assert status == 0 and tr.same_bits(host(c.body_template_vertices), vtn[None])
    idx, sw = sparse_skin_weights(b.skin_weights, rows=c.nn_ids)
    assert torch.equal(c.skin_idx, idx) and torch.equal(c.skin_w, sw)
    assert torch.equal(b.skin_weights[c.nn_ids], torch.zeros_like(b.skin_weights[c.nn_ids]).scatter_(1, idx.long(), sw))
    # a step of lbs_cage from the binding at the star pose reproduces the cage that was bound
    posed = lbs_cage(c.body_template_vertices[0], bs[0][c.nn_ids], A[0], c.skin_idx, c.skin_w)
    np.testing.assert_allclose(host(posed), cage, rtol=1e-5, atol=1e-5 * float(np.abs(cage).max()))


def test_bind_cage_skin():
    from d3ga_amd import bind_cage_skin
    v, f = mesh("sphere128")
    rng = np.random.default_rng(3)
    cage = (v[rng.integers(0, len(v), 100)] * 1.2).astype(np.float32)
    w, idx = torch.rand(len(v), 8, device=DEV), torch.randint(0, 30, (len(v), 8), device=DEV)
    cw, ci, ids = bind_cage_skin(dev(v), dev(f), dev(cage), 0.0, w, idx)
    assert np.array_equal(host(ids), tr.nearest(v, cage)) and torch.equal(cw, w[ids]) and torch.equal(ci, idx[ids])
