"""Cage surface authoring on the GPU (d3ga_amd/cage_author.py, csrc/cage_author.hip): the kernels against the g++ build of
csrc/cage_author_math.h (tests/cage_author_ref.py) -- bit for bit for grids, isosurface and labels, to 2^-23 max|x| for the
smoothers (acos is the one library call) -- at the smallest shapes that can still go wrong: grids of 13^3 to 65^3, x rows that end
inside and just past a 64-bit word, counts on a scan block's boundary.  The g++ build itself is held to the numpy / scipy oracle
and to first principles in tests/test_cage_author_host.py."""
import numpy as np
import pytest
import torch

import cage_author_ref as cr

pytestmark = pytest.mark.gpu
DEV = "cuda"
SMOOTH_BOUND = 2.0 ** -23
_CACHE = {}


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.detach().cpu().numpy()


def shared(key, make):
    """references are computed once and never written to"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def grid_of(dense):
    from d3ga_amd import VoxelGrid
    return VoxelGrid.from_dense(dev(dense))


@pytest.mark.parametrize("radius", [6, 31, 32])
def test_voxelize_equals_the_host_build(radius):
    from d3ga_amd import voxelize
    for name, v, f in cr.voxel_cases(radius):
        want, _ = shared(("surface", radius, name), lambda: cr.host_surface(v, f, radius))
        got = voxelize(dev(v), dev(f), radius, fill=False)
        assert got.rounds is None and (got.radius, got.D, got.W) == (radius, 2 * radius + 1, (2 * radius + 64) // 64)
        assert np.array_equal(host(got.bits).view(np.uint64), cr.pack(want)), name             # also: no bit beyond a row's end
        assert np.array_equal(host(got.dense()), want), name
        filled = voxelize(dev(v.astype(np.float32)).double(), dev(f).long(), radius)           # float32-born vertices, int64 faces
        assert filled.rounds >= 1
    v, f = next((v, f) for name, v, f in cr.voxel_cases(radius) if name == "a sphere")
    want_filled, rounds = shared(("filled sphere", radius), lambda: cr.host_fill(cr.host_surface(v, f, radius)[0]))
    got = voxelize(dev(v), dev(f), radius, fill=True)
    assert np.array_equal(host(got.dense()), want_filled) and got.rounds == rounds and want_filled.sum() > cr.host_surface(v, f, radius)[0].sum()


def _fill_cases():
    yield "a nested shell", cr.shell_grid(10)
    yield "an open bowl", cr.bowl_grid(10)
    yield "a serpentine corridor", cr.serpentine_grid(10)
    yield "an empty grid", np.zeros((13, 13, 13), bool)
    yield "a mesh that touches the border", cr.host_surface(*list(cr.voxel_cases(6))[3][1:], 6)[0]
    for radius in (31, 32):
        g = cr.shell_grid(radius)
        yield f"a shell at radius {radius}", g.copy()
        g[radius + radius // 2:, radius, radius] = False
        yield f"a tunnelled shell at radius {radius}", g


@pytest.mark.parametrize("case", range(9))
def test_fill_equals_scipy(case):
    from d3ga_amd import fill_holes
    name, g = list(_fill_cases())[case]
    want, rounds = shared(("fill", name), lambda: cr.host_fill(g))
    assert np.array_equal(want, cr.fill(g)), name              # scipy.ndimage.binary_fill_holes itself
    got = fill_holes(grid_of(g))
    assert np.array_equal(host(got.dense()), want) and got.rounds == rounds, name
    assert np.array_equal(host(got.bits).view(np.uint64), cr.pack(want)), name
    if name == "a serpentine corridor":
        assert g.shape[0] == 21 and got.rounds > 1
    if name in ("an open bowl", "an empty grid") or "tunnelled" in name:
        assert int(got.dense().sum()) == int(g.sum()), name       # nothing is filled
    if name == "a nested shell":
        assert int(got.dense().sum()) > int(g.sum())           # the cavity is
    lazy = fill_holes(grid_of(g), check_every=4)               # reading back every fourth round: the same bits
    assert torch.equal(lazy.bits, got.bits) and lazy.rounds % 4 == 0 and lazy.rounds >= got.rounds


def _iso_cases():
    edge, corner = np.zeros((13, 13, 13), bool), np.zeros((13, 13, 13), bool)
    edge[5, 5, 5] = edge[6, 6, 5] = corner[5, 5, 5] = corner[6, 6, 6] = True
    yield "a full grid", np.ones((13, 13, 13), bool)
    yield "two voxels touching at an edge", edge
    yield "two voxels touching at a corner", corner
    yield "256 crossed edges", cr.counted_grid(6, 9, 5)
    yield "258 crossed edges", cr.counted_grid(6, 11, 4)
    yield "a 50 % random grid", np.random.default_rng(0).random((17, 17, 17)) < 0.5
    yield "a torus", cr.torus_grid(10)
    yield "a ball at radius 31", cr.ball(31, 9.3, (20, 3, -7))
    yield "a ball at radius 32", cr.ball(32, 9.3, (20, 3, -7))


@pytest.mark.parametrize("case", range(9))
def test_isosurface_equals_the_host_build(case):
    """A crossed-edge count is always even, so the grid one past the scan block of 256 is the one with 258
    (tests/test_cage_author_host.py::test_isosurface)."""
    from d3ga_amd import isosurface
    name, g = list(_iso_cases())[case]
    centre, scale = (0.25, -1.5, 0.125), (0.8, 0.8, 1.0)
    want_v, want_f = shared(("iso", name), lambda: cr.host_isosurface(g, centre, scale))
    v, f = isosurface(grid_of(g), centre=torch.tensor(centre, dtype=torch.float64, device=DEV), scale=scale)
    assert v.dtype == torch.float32 and f.dtype == torch.int32
    assert cr.same_bits(host(v), want_v) and np.array_equal(host(f), want_f), name
    if "crossed edges" in name:
        assert len(v) == int(name.split()[0])
    plain = isosurface(grid_of(g))
    assert np.array_equal(host(plain[1]), want_f) and cr.same_bits(host(plain[0]), cr.host_isosurface(g)[0])
    two, once, _ = cr.edge_census(host(f))
    assert two and once


def test_isosurface_of_an_empty_grid():
    from d3ga_amd import VoxelGrid, isosurface
    v, f = isosurface(VoxelGrid.empty(6))
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3) and v.dtype == torch.float32 and f.dtype == torch.int32


def _smooth_mesh(name):
    return shared(("mesh", name), lambda: cr.mesh_of(cr.ellipsoid_grid(8), 1, 0.004) if name == "ellipsoid" else cr.mesh_of(cr.torus_grid(10), 2, 0.004))


@pytest.mark.parametrize("name", ["ellipsoid", "torus"])
@pytest.mark.parametrize("num_iter", [1, 25])
def test_smoothers_equal_the_host_build(name, num_iter):
    """|device - host build| <= 2^-23 max|x|: the same float64 text with one float32 rounding; acos is the one library call, and
    the inputs are in general position (tests/test_cage_author_host.py::test_smoothers asserts the conditions)."""
    from d3ga_amd import loop_plan, smooth_improved, smooth_taubin
    v, f = _smooth_mesh(name)
    want, st = shared(("improved", name, num_iter), lambda: cr.host_smooth(cr.IMPROVED, v, f, num_iter, 0.25))
    got = smooth_improved(dev(v), dev(f), num_iter=num_iter, lbd=0.25)
    worst = np.abs(host(got.vertices).astype(np.float64) - want).max() / np.abs(want).max()
    print(f"{name} improved x{num_iter}: worst {worst / SMOOTH_BOUND:.3f} of the bound")
    assert st == 0 and got.check() is got and got.vertices.dtype == torch.float32 and worst <= SMOOTH_BOUND
    plan = loop_plan(dev(f), len(v))
    again = smooth_improved(dev(v), dev(f), num_iter=num_iter, lbd=0.25, plan=plan)            # the plan passed in: equal bits
    assert torch.equal(again.vertices, got.vertices) and torch.equal(smooth_improved(dev(v), dev(f), num_iter, 0.25, plan=plan).vertices, got.vertices)
    want, st = shared(("taubin", name, num_iter), lambda: cr.host_smooth(cr.TAUBIN, v, f, num_iter, 0.5, -0.53))
    got = smooth_taubin(dev(v), dev(f), iterations=num_iter, plan=plan)
    assert st == 0 and np.abs(host(got.check().vertices).astype(np.float64) - want).max() <= SMOOTH_BOUND * np.abs(want).max()
    assert cr.same_bits(host(got.vertices), want)               # no library call in this one: the same bits
    assert torch.equal(smooth_taubin(dev(v), dev(f), iterations=num_iter).vertices, got.vertices)


def test_smoothers_flag_an_isolated_vertex():
    from d3ga_amd import smooth_improved, smooth_taubin
    v, f = cr.mesh_of(cr.ball(6), 1, 0.004)
    lone = np.concatenate([v, [[0.3, 0.2, 0.1]]])
    for fn, mode in ((lambda: smooth_improved(dev(lone), dev(f), num_iter=2, lbd=0.25), cr.IMPROVED), (lambda: smooth_taubin(dev(lone), dev(f), iterations=2), cr.TAUBIN)):
        got = fn()
        want, st = cr.host_smooth(mode, lone, f, 2, 0.25 if mode == cr.IMPROVED else 0.5, -0.53)
        assert st == cr.STATUS_ISOLATED and int(got.status.item()) == st
        with pytest.raises(ValueError, match="no face or no neighbour"):
            got.check()
        out = host(got.vertices)
        assert np.isfinite(out).all() and out[-1].tolist() == lone[-1].astype(np.float32).tolist()
        assert np.abs(out.astype(np.float64) - want).max() <= SMOOTH_BOUND * np.abs(want).max()


def test_components():
    from d3ga_amd import face_components, keep_components, loop_plan
    g = cr.ball(10, 6.0)
    g[18, 18, 18] = True                                      # a single-voxel blob: 24 faces, fewer than 70
    v, f = shared(("mesh", "ball + blob"), lambda: cr.mesh_of(g))
    want = shared(("labels", "ball + blob"), lambda: cr.host_components(f, len(v)))
    labels = face_components(dev(f), len(v))
    assert labels.dtype == torch.int32 and np.array_equal(host(labels), want) and sorted(np.unique(want, return_counts=True)[1].tolist()) == [24, len(f) - 24]
    plan = loop_plan(dev(f), len(v))
    assert torch.equal(face_components(dev(f).long(), len(v), plan=plan), labels)
    kv, kf = keep_components(dev(v.astype(np.float32)), dev(f), min_faces=70)
    wv, wf = cr.keep_components(v.astype(np.float32), f, 70, True, want)
    assert kv.dtype == torch.float32 and kf.dtype == torch.int32 and cr.same_bits(host(kv), wv) and np.array_equal(host(kf), wf)
    assert len(kf) == len(f) - 24 and len(kv) == len(v) - 14                                   # the blob is dropped, the vertices compacted
    av, af = keep_components(dev(v), dev(f), min_faces=0)
    assert len(af) == len(f) and len(av) == len(v) and av.dtype == torch.float64 and np.array_equal(host(af), f)
    uv, uf = keep_components(dev(v), dev(f), min_faces=70, drop_unreferenced=False)
    assert len(uv) == len(v) and torch.equal(uv[uf.long()].float(), kv[kf.long()])
    fv, ff = keep_components(dev(v), dev(f[:, [0, 2, 1]]), min_faces=70)                        # inside out: every face flipped back
    assert cr.signed_volume(host(fv), host(ff)) > 0 and np.array_equal(np.sort(host(ff), 1), np.sort(wf, 1))
    # label equality on the torus and on a surface of many parts
    for name, grid in (("torus", cr.torus_grid(10)), ("random", np.random.default_rng(0).random((17, 17, 17)) < 0.5)):
        tv, tf = shared(("mesh", name), lambda: cr.mesh_of(grid))
        assert np.array_equal(host(face_components(dev(tf), len(tv))), shared(("labels", name), lambda: cr.host_components(tf, len(tv)))), name


def test_cage_processor_end_to_end():
    """The device's chain against the chain of host-build stages fed with the device's prepared vertices (`prepare` is
    `gauss_init.inflate`, which has tests of its own): identical grids and faces, vertices within the smoother bound; two calls
    give identical bits; every vertex of the input mesh lies inside the result, read off the filled grid."""
    from d3ga_amd import cage_processor, create_cage, prepare, voxelize
    v, f = shared(("mesh", "figure"), cr.capsule_figure)
    radius, inflate, scale = 16, 0.01, 0.8
    pv, centre = prepare(dev(v), dev(f), inflate, scale)
    assert pv.dtype == torch.float64 and float(pv.mean(0).abs().max()) < 1e-12
    want_v, want_f, want_grid = shared(("chain",), lambda: cr.host_chain(host(pv), f, radius, host(centre), scale))
    grid = voxelize(pv, dev(f), radius, fill=True)
    assert np.array_equal(host(grid.dense()), want_grid)
    cv, cf = create_cage(dev(v), dev(f), radius, inflate, scale)
    hv, hf = cr.host_isosurface(want_grid, host(centre), (scale, scale, 1.0))
    assert cr.same_bits(host(cv), hv) and np.array_equal(host(cf), hf)
    out_v, out_f = cage_processor(dev(v), dev(f), cage_tris_target=0, radius=radius, inflate=inflate)
    assert out_v.dtype == torch.float32 and out_f.dtype == torch.int64 and out_v.shape[0] == 1 and out_f.shape[0] == 1 and out_v.is_cuda
    assert np.array_equal(host(out_f[0]), want_f) and len(want_f) >= 70
    assert np.abs(host(out_v[0]).astype(np.float64) - want_v).max() <= SMOOTH_BOUND * np.abs(want_v).max()
    again_v, again_f = cage_processor(dev(v), dev(f), 0, radius, inflate)
    assert torch.equal(again_v, out_v) and torch.equal(again_f, out_f)

    class Mesh:
        vertices, faces = v, f
    obj_v, obj_f = cage_processor(Mesh(), radius=radius)         # an object with .vertices and .faces (numpy arrays are uploaded)
    assert torch.equal(obj_v, out_v) and torch.equal(obj_f, out_f)
    # inside: the voxel that holds each prepared input vertex is occupied in the filled grid the surface was cut from
    idx = np.floor(host(pv) / cr.pitch(radius) + radius + 0.5).astype(np.int64)
    assert ((idx >= 0) & (idx < 2 * radius + 1)).all() and want_grid[tuple(idx.T)].all()
    two, once, _ = cr.edge_census(host(out_f[0]))
    assert two and once and cr.signed_volume(host(out_v[0]), host(out_f[0])) > 0
    with pytest.raises(NotImplementedError, match="quadric decimation is not built yet"):
        cage_processor(dev(v), dev(f), cage_tris_target=5000)
