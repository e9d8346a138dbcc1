"""Cage surface authoring without a GPU: the g++ build of csrc/cage_author_math.h -- the text the kernels run -- against the
numpy / scipy oracle (tests/cage_author_ref.py), exactly for grids, isosurface and labels and to 2^-23 max|x| for the smoothers;
first-principles checks that use no oracle; the Python layer's ValueErrors and NotImplementedError; the ABI surface and its
refusals.  Parity with trimesh, mcubes and open3d is unpinned: the project depends on none of them, so no golden exists."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import cage_author_ref as cr
import template_bind_ref as tr
from conftest import ROOT

E_NULL, E_SIZE, E_CONFIG, E_CAPACITY = -1, -2, -3, -4        # D3GA_E_* (include/d3ga.h)
ENTRY_POINTS = (("d3ga_cage_voxelize", 7), ("d3ga_cage_fill", 6), ("d3ga_cage_iso_scratch_bytes", 2), ("d3ga_cage_iso_count", 5),
                ("d3ga_cage_iso_emit", 5), ("d3ga_cage_smooth", 3), ("d3ga_cage_components", 5))
SMOOTH_BOUND = 2.0 ** -23                                    # |a - b| <= 2^-23 max|b|: float64 arithmetic, one float32 rounding, acos the one library call


def _samples(tri, n=24):
    """dense barycentric samples of one triangle (3,3), its corners and edges included"""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    keep = i + j <= n
    a, b = i[keep] / n, j[keep] / n
    return tri[0] + a[:, None] * (tri[1] - tri[0]) + b[:, None] * (tri[2] - tri[0])


@pytest.mark.parametrize("radius", [6, 31, 32])
def test_surface_voxels(radius):
    """The g++ build equals the oracle on every case; and, with no oracle: every voxel that holds a sample point of a triangle is
    set, and every set voxel's centre lies within (sqrt(3) / 2) pitch (1 + 2^-40) of some triangle."""
    pt, D = cr.pitch(radius), 2 * radius + 1
    for name, v, f in cr.voxel_cases(radius):
        if radius > 6 and name in ("a triangle larger than the grid", "a mesh that touches the border"):
            continue                                          # the numpy oracle walks every voxel of the box: kept to the small grid
        got, status = cr.host_surface(v, f, radius)
        assert status == 0 and np.array_equal(got, cr.surface(v, f, radius)), name
        tris = v[f]
        for tri in tris:
            p = _samples(tri)
            # a sample strictly inside one voxel (not within 1e-9 pitch of a voxel face) names that voxel without doubt
            q = p / pt + radius + 0.5
            sure = (np.abs(q - np.round(q)) > 1e-9).all(1)
            idx = np.floor(q[sure]).astype(np.int64)
            idx = idx[((idx >= 0) & (idx < D)).all(1)]
            assert got[tuple(idx.T)].all(), name
        centres = (np.argwhere(got) - radius) * pt
        assert len(centres) > 0 or name == "nothing"
        assert (cr.point_triangle_distance(centres, tris) <= np.sqrt(3) / 2 * pt * (1 + 2.0 ** -40)).all(), name
    # the fixed cases, said out loud
    cases = {name: (v, f) for name, v, f in cr.voxel_cases(radius)}
    assert cr.host_surface(*cases["a triangle inside one voxel"], radius)[0].sum() == 1
    on_face = cr.host_surface(*cases["a vertex on a voxel face"], radius)[0]
    assert on_face[radius, radius, radius] and on_face[radius + 1, radius, radius]       # closed cubes: both sides of the face
    line = cr.host_surface(*cases["a zero-area triangle"], radius)[0]
    assert line[radius, radius, radius] and line.sum() >= 0.6 / pt                       # the segment and the point
    if radius == 6:
        assert cr.host_surface(*cases["a triangle larger than the grid"], radius)[0][:, :, radius].all()
    # a face that names a vertex outside the mesh is left out and flagged
    v, f = cases["a sphere"]
    bad = np.concatenate([f, [[0, 1, len(v)]]]).astype(np.int32)
    got, status = cr.host_surface(v, bad, radius)
    assert status == cr.STATUS_RANGE and np.array_equal(got, cr.host_surface(v, f, radius)[0])


def _fill_cases():
    yield "a nested shell", cr.shell_grid(10), None
    yield "an open bowl", cr.bowl_grid(10), 0
    yield "a serpentine corridor", cr.serpentine_grid(10), 0
    yield "an empty grid", np.zeros((13, 13, 13), bool), 0
    yield "a mesh that touches the border", cr.surface(*list(cr.voxel_cases(6))[3][1:], 6), None
    for radius in (31, 32):                                  # an x row ends inside, and just past, one 64-bit word
        g = cr.shell_grid(radius)
        g[radius + radius // 2:, radius, radius] = False        # a tunnel from the cavity to the border at the row's end: nothing is filled
        yield f"a tunnelled shell at radius {radius}", g, 0
        yield f"a shell at radius {radius}", cr.shell_grid(radius), None


def test_fill_is_binary_fill_holes():
    for name, g, added in _fill_cases():
        got, rounds = cr.host_fill(g)
        want = cr.fill(g)
        assert np.array_equal(got, want), name
        if added is not None:
            assert got.sum() - g.sum() == added, name
        else:
            assert got.sum() > g.sum(), name
        if name == "a serpentine corridor":
            assert g.shape[0] == 21 and rounds > 1, rounds
    # the definition, with no oracle: what is not filled is the empty voxels 6-connected to the border
    g = cr.shell_grid(10)
    import scipy.ndimage as ndi
    lab, _ = ndi.label(~g)
    border = np.ones_like(g)
    border[1:-1, 1:-1, 1:-1] = False
    outside = np.isin(lab, np.unique(lab[border & ~g]))
    assert np.array_equal(cr.host_fill(g)[0], ~outside)


def _iso_cases():
    edge, corner = np.zeros((13, 13, 13), bool), np.zeros((13, 13, 13), bool)
    edge[5, 5, 5] = edge[6, 6, 5] = corner[5, 5, 5] = corner[6, 6, 6] = True
    yield "a ball", cr.ball(6), 2
    yield "a torus", cr.torus_grid(10), 0
    yield "an unfilled shell", cr.shell_grid(10), 4
    yield "a full grid", np.ones((13, 13, 13), bool), 2
    yield "two voxels touching at an edge", edge, None
    yield "two voxels touching at a corner", corner, None
    yield "256 crossed edges", cr.counted_grid(6, 9, 5), None
    yield "258 crossed edges", cr.counted_grid(6, 11, 4), None
    yield "a 50 % random grid", np.random.default_rng(0).random((17, 17, 17)) < 0.5, None
    yield "a ball at radius 32", cr.ball(32, 9.3, (20, 3, -7)), 2


def test_isosurface():
    """Equal to the oracle exactly; and, with no oracle: every vertex is the midpoint of a grid edge with one occupied and one
    empty end, every undirected edge is in exactly two faces and every directed edge appears once, V - E + F is the surface's, and
    the signed volume is positive.  A crossed-edge count is always even (14 Kuhn edges end at every occupied lattice point, an
    edge inside takes two away), so the grid `one past` the scan block of 256 is the one with 258."""
    for name, g, chi in _iso_cases():
        v, f = cr.host_isosurface(g)
        ov, of, edges = cr.isosurface(g)
        assert cr.same_bits(v, ov) and np.array_equal(f, of) and f.dtype == np.int32, name
        D = g.shape[0]
        radius = (D - 1) // 2
        pad = np.zeros((D + 2,) * 3, bool)
        pad[1:-1, 1:-1, 1:-1] = g
        lo, hi = edges[:, 0], edges[:, 1]
        assert (pad[tuple((lo + 1).T)] != pad[tuple((hi + 1).T)]).all() and ((hi - lo >= 0) & (hi - lo <= 1)).all() and (hi != lo).any(1).all(), name
        assert np.array_equal(v, (((lo + hi) / 2.0) / radius - 1.0).astype(np.float32)), name
        two, once, n_edges = cr.edge_census(f)
        assert two and once and len(np.unique(f)) == len(v), name
        assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 0] != f[:, 2]).all(), name
        if chi is not None:
            assert len(v) - n_edges + len(f) == chi, name
        assert cr.signed_volume(v, f) > 0, name
        if "crossed edges" in name:
            assert len(v) == int(name.split()[0])
    v, f = cr.host_isosurface(np.ones((13, 13, 13), bool))     # the padded box: every vertex half a voxel outside one of the grid's six sides
    x = (v.astype(np.float64) + 1.0) * 6
    assert (np.isclose(x, -0.5) | np.isclose(x, 12.5)).any(1).all() and np.isclose(x.min(0), -0.5).all() and np.isclose(x.max(0), 12.5).all()
    assert 12.0 ** 3 < cr.signed_volume(x, f) < 13.0 ** 3                                 # it holds the lattice points' hull and lies in the padded box
    v, f = cr.host_isosurface(np.zeros((13, 13, 13), bool))
    assert v.shape == (0, 3) and f.shape == (0, 3)
    # the map back: ((x / radius - 1) + centre) / scale, one rounding
    g, c, s = cr.ball(6), (0.25, -1.5, 0.125), (0.8, 0.8, 1.0)
    v, f = cr.host_isosurface(g, c, s)
    ov, of, _ = cr.isosurface(g, c, s)
    assert cr.same_bits(v, ov) and np.array_equal(f, of)


def _smooth_meshes():
    yield "ellipsoid", cr.mesh_of(cr.ellipsoid_grid(8), 1, 0.004)
    yield "torus", cr.mesh_of(cr.torus_grid(10), 2, 0.004)


@pytest.mark.parametrize("num_iter", [1, 25])
def test_smoothers(num_iter):
    """The bound's conditions on the inputs, then the bound: the oracle's own spread when every acos moves by one ulp stays below
    2^-40, no `inner >= 0` branch flips, no vertex has |inner| <= 1e-9 |dot|."""
    for name, (v, f) in _smooth_meshes():
        want, exact, branches, margin = cr.smooth_improved(v, f, num_iter, 0.25, details=True)
        _, moved, flipped, _ = cr.smooth_improved(v, f, num_iter, 0.25, perturb=np.random.default_rng(5), details=True)
        assert np.abs(exact - moved).max() < 2.0 ** -40 and np.array_equal(branches, flipped) and margin > 1e-9, name
        assert len(v) == (1390 if name == "ellipsoid" else len(v))
        got, status = cr.host_smooth(cr.IMPROVED, v, f, num_iter, 0.25)
        worst = np.abs(got.astype(np.float64) - want).max() / np.abs(want).max()
        print(f"{name} improved x{num_iter}: worst {worst / SMOOTH_BOUND:.3f} of the bound")
        assert status == 0 and worst <= SMOOTH_BOUND, name
        got, status = cr.host_smooth(cr.TAUBIN, v, f, num_iter, 0.5, -0.53)
        want = cr.smooth_taubin(v, f, num_iter)
        assert status == 0 and np.abs(got.astype(np.float64) - want).max() <= SMOOTH_BOUND * np.abs(want).max(), name
        assert got.dtype == np.float32 and np.abs(got - v).max() > 1e-4                     # it moved


def test_smoothers_flag_what_the_reference_turns_into_nan():
    v, f = cr.mesh_of(cr.ball(6), 1, 0.004)
    lone = np.concatenate([v, [[0.3, 0.2, 0.1]]])
    for mode in (cr.IMPROVED, cr.TAUBIN):
        got, status = cr.host_smooth(mode, lone, f, 2, 0.25, -0.2)
        assert status == cr.STATUS_ISOLATED and got[-1].tolist() == lone[-1].astype(np.float32).tolist() and np.isfinite(got).all()
        assert cr.same_bits(got[:-1], cr.host_smooth(mode, v, f, 2, 0.25, -0.2)[0])
    twin = v.copy()
    twin[f[0, 1]] = twin[f[0, 0]]
    got, status = cr.host_smooth(cr.IMPROVED, twin, f, 1, 0.25)
    assert status & cr.STATUS_ZERO_EDGE and np.isfinite(got).all()


def test_components():
    g = cr.ball(10, 6.0)
    g[18, 18, 18] = True                                      # a single-voxel blob: 24 faces (the 24 tetrahedra at its lattice point)
    v, f = cr.mesh_of(g)
    for name, faces, n in (("ball + blob", f, len(v)), ("torus", cr.mesh_of(cr.torus_grid(10))[1], None), ("random", cr.mesh_of(np.random.default_rng(0).random((17, 17, 17)) < 0.5)[1], None),
                           ("shuffled", tr.shuffled(v, f, 3)[1], len(v))):
        n = int(faces.max()) + 1 if n is None else n
        want = cr.components(faces)
        assert np.array_equal(cr.host_components(faces, n), want), name
        for part in np.unique(want):
            assert part == np.nonzero(want == part)[0].min()
    labels = cr.components(f)
    sizes = np.unique(labels, return_counts=True)[1]
    assert sorted(sizes.tolist()) == [24, len(f) - 24]
    kv, kf = cr.keep_components(v, f, 70)
    assert len(kf) == len(f) - 24 and len(kv) == len(v) - 14 and cr.edge_census(kf)[:2] == (True, True) and cr.signed_volume(kv, kf) > 0
    av, af = cr.keep_components(v, f, 0)
    assert len(af) == len(f) and len(av) == len(v)
    uv, uf = cr.keep_components(v, f, 70, drop_unreferenced=False)
    assert len(uv) == len(v) and np.array_equal(uv[uf], kv[kf])
    fv, ff = cr.keep_components(v, f[:, [0, 2, 1]], 70)         # inside out: flipped back
    assert np.array_equal(ff, kf) and np.array_equal(fv, kv) and cr.signed_volume(fv, ff) > 0


class _Mesh:
    def __init__(self, vertices, faces):
        self.vertices, self.faces = vertices, faces


def test_python_layer_refuses_bad_input():
    from d3ga_amd import _lib, cage_author as ca
    v, f = (torch.from_numpy(x) for x in cr.mesh_of(cr.ball(6)))
    nan_v = v.clone()
    nan_v[3, 1] = float("nan")
    grid = ca.VoxelGrid(6, torch.zeros((13, 13, 1), dtype=torch.int64))
    bad = [
        lambda: ca.voxelize(v, f, radius=0), lambda: ca.voxelize(v, f, radius=512), lambda: ca.voxelize(v, f, radius=6.0), lambda: ca.voxelize(v, f, radius=True),
        lambda: ca.voxelize(v[:, :2], f, 6), lambda: ca.voxelize(v, f.float(), 6), lambda: ca.voxelize(nan_v, f, 6), lambda: ca.voxelize(v, f + len(v), 6),
        lambda: ca.voxelize(v, None, 6), lambda: ca.voxelize("mesh", None, 6), lambda: ca.voxelize(v.half(), f, 6), lambda: ca.voxelize(v, f.to("meta"), 6),
        lambda: ca.prepare(v, f, inflate=float("nan")), lambda: ca.prepare(v, f, scale=0.0), lambda: ca.prepare(v, f, scale=-1.0), lambda: ca.prepare(v, f, scale="0.8"),
        lambda: ca.fill_holes("grid"), lambda: ca.fill_holes(grid, check_every=0), lambda: ca.isosurface("grid"), lambda: ca.isosurface(grid, centre=[0.0, 1.0]),
        lambda: ca.isosurface(grid, scale=0.0), lambda: ca.isosurface(grid, centre=[0.0, float("inf"), 0.0]),
        lambda: ca.VoxelGrid(6, torch.zeros((13, 13, 2), dtype=torch.int64)), lambda: ca.VoxelGrid(6, torch.zeros((13, 13, 1), dtype=torch.int32)),
        lambda: ca.VoxelGrid.from_dense(torch.zeros((12, 12, 12), dtype=torch.bool)), lambda: ca.VoxelGrid.from_dense(torch.zeros((13, 13, 13))),
        lambda: ca.smooth_improved(v, f, num_iter=0), lambda: ca.smooth_improved(v, f, num_iter=2.5), lambda: ca.smooth_improved(v, f, lbd=float("inf")),
        lambda: ca.smooth_improved(v, f, plan="plan"), lambda: ca.smooth_improved(nan_v, f), lambda: ca.smooth_taubin(v, f, iterations=-1),
        lambda: ca.smooth_taubin(v, f, mu=float("nan")), lambda: ca.smooth_taubin(v, f, iterations=4097),
        lambda: ca.face_components(f, 0), lambda: ca.face_components(f, 2.0), lambda: ca.face_components(f.float(), len(v)), lambda: ca.face_components(f[:, :2], len(v)),
        lambda: ca.keep_components(v, f, min_faces=-1), lambda: ca.keep_components(v, f, min_faces=1.5), lambda: ca.simplify(v, f, tris_target=-3),
        lambda: ca.cage_processor(v, f, cage_tris_target=1.5), lambda: ca.cage_processor(v, f, radius=0), lambda: ca.create_cage(v, f, scale=0),
    ]
    for i, fn in enumerate(bad):
        with pytest.raises(ValueError):
            fn()
            pytest.fail(f"case {i} was accepted")
    # decimation is the next piece of work: an explicit refusal, before anything is launched
    for fn in (lambda: ca.simplify(v, f, 5000), lambda: ca.cage_processor(v, f, cage_tris_target=5000), lambda: ca.cage_processor(_Mesh(v, f), None, 1)):
        with pytest.raises(NotImplementedError, match="quadric decimation is not built yet; choose `radius` for the triangle count or decimate outside"):
            fn()
    # everything fits, but the tensors live on the CPU: no fallback, and nothing was launched
    ok = [lambda: ca.voxelize(v, f, 6), lambda: ca.voxelize(_Mesh(v, f), radius=6, fill=False), lambda: ca.prepare(v.float(), f.long()), lambda: ca.fill_holes(grid),
          lambda: ca.isosurface(grid), lambda: ca.smooth_improved(v, f), lambda: ca.smooth_taubin(v[None], f[None]), lambda: ca.face_components(f, len(v)),
          lambda: ca.keep_components(v, f), lambda: ca.create_cage(v, f), lambda: ca.smooth_cage(_Mesh(v, f)), lambda: ca.simplify(v, f, 0), lambda: ca.cage_processor(v, f)]
    for fn in ok:
        with pytest.raises(_lib.D3GAError):
            fn()
    if not torch.cuda.is_available():
        with pytest.raises(_lib.D3GAError):
            ca.voxelize(v.numpy(), f.numpy(), 6)             # arrays are uploaded: without a GPU that is the package's usual error
    # what the status word turns into
    for bit, text in ((_lib.CAGE_STATUS_RANGE, "outside"), (_lib.CAGE_STATUS_ISOLATED, "no face or no neighbour"), (_lib.CAGE_STATUS_ZERO_EDGE, "length 0")):
        with pytest.raises(ValueError, match=text):
            ca.Smoothed(v, torch.tensor([bit], dtype=torch.int32)).check()
    s = ca.Smoothed(v, torch.zeros(1, dtype=torch.int32))
    assert s.check() is s and tuple(s)[0] is v
    # the bit layout, on the CPU: dense() and from_dense() are each other's inverse and agree with the oracle's packing
    for D in (13, 63, 65):
        dense = np.random.default_rng(D).random((D, D, D)) < 0.3
        g = ca.VoxelGrid.from_dense(torch.from_numpy(dense))
        assert g.radius == (D - 1) // 2 and np.array_equal(g.bits.numpy().view(np.uint64), cr.pack(dense)) and np.array_equal(g.dense().numpy(), dense)
    assert grid.pitch == cr.pitch(6)


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
    for name, value in (("STATUS_RANGE", cr.STATUS_RANGE), ("STATUS_ISOLATED", cr.STATUS_ISOLATED), ("STATUS_ZERO_EDGE", cr.STATUS_ZERO_EDGE),
                        ("FILL_BEGIN", cr.FILL_BEGIN), ("FILL_ROUND", cr.FILL_ROUND), ("FILL_FINISH", cr.FILL_FINISH), ("SMOOTH_IMPROVED", cr.IMPROVED),
                        ("SMOOTH_TAUBIN", cr.TAUBIN), ("PARTS_BEGIN", cr.PARTS_BEGIN), ("PARTS_ROUND", cr.PARTS_ROUND), ("MAX_RADIUS", 511), ("MAX_ITERATIONS", 4096)):
        assert getattr(_lib, "CAGE_" + name) == value and re.search(r"#define\s+D3GA_CAGE_%s\s+%d\b" % (name, value), src), name
    for ours, theirs in ((_lib.VoxelGridDesc, cr.GridStruct), (_lib.CageIsoDesc, cr.IsoStruct), (_lib.CageSmoothDesc, cr.SmoothStruct)):
        assert ctypes.sizeof(ours) == ctypes.sizeof(theirs) and [n for n, _ in ours._fields_] == [n for n, _ in theirs._fields_]
    assert ctypes.sizeof(_lib.VoxelGridDesc) == 24 and ctypes.sizeof(_lib.CageIsoDesc) == 8 + 48 + 16 and ctypes.sizeof(_lib.CageSmoothDesc) == 24 + 64
    build = open(os.path.join(ROOT, "d3ga_amd", "csrc", "build.py")).read()
    assert "cage_author.hip" in build and "cage_author_math.h" in build and 'EXTRA["cage_author.hip"] = ["-ffp-contract=off"]' in build
    import d3ga_amd
    from d3ga_amd import cage_author
    for name in cage_author.__all__:
        assert name in d3ga_amd.__all__ and getattr(d3ga_amd, name) is getattr(cage_author, name)
    n = ctypes.c_int64(-1)
    L = _lib.lib()
    for radius in (1, 6, 32, 120, 511):
        assert L.d3ga_cage_iso_scratch_bytes(radius, ctypes.byref(n)) == 0 and n.value == cr.lib().hc_cage_iso_scratch_bytes(radius)
        N = (2 * radius + 2) ** 3
        assert n.value % 256 == 0 and n.value >= 4 * N + 24 * ((N + 255) // 256 + 1)
    for radius in (0, -5, 512):
        assert L.d3ga_cage_iso_scratch_bytes(radius, ctypes.byref(n)) == E_SIZE and cr.lib().hc_cage_iso_scratch_bytes(radius) == E_SIZE
    assert L.d3ga_cage_iso_scratch_bytes(6, None) == E_NULL


@pytest.mark.parametrize("which", ["library", "host build"])
def test_entry_points_refuse_bad_arguments_before_any_launch(which):
    """The refusals happen before any HIP call: host buffers stand in for device memory and are never touched.  The g++ build runs
    the same check functions and must give the same statuses."""
    from d3ga_amd import _lib
    buf = (ctypes.c_uint8 * 8192)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) & ~255)
    at = lambda k: ctypes.c_void_p(p.value + k)
    if which == "library":
        L, tail = _lib.lib(), (None,)
        G, I, S, P = _lib.VoxelGridDesc, _lib.CageIsoDesc, _lib.CageSmoothDesc, _lib.LoopPlanTables
        vox, fill, count, emit, smooth, parts = L.d3ga_cage_voxelize, L.d3ga_cage_fill, L.d3ga_cage_iso_count, L.d3ga_cage_iso_emit, L.d3ga_cage_smooth, L.d3ga_cage_components
    else:
        L, tail = cr.lib(), ()
        G, I, S, P = cr.GridStruct, cr.IsoStruct, cr.SmoothStruct, tr.PlanStruct
        vox, fill, count, emit, smooth, parts = L.hc_cage_voxelize, L.hc_cage_fill, L.hc_cage_iso_count, L.hc_cage_iso_emit, L.hc_cage_smooth, L.hc_cage_components
    grid = lambda **kw: ctypes.byref(G(**{**dict(radius=6, D=13, W=1, reserved=0, bits=p.value), **kw}))
    bad_grids = ((dict(radius=0, D=1), E_SIZE), (dict(radius=512, D=1025, W=17), E_SIZE), (dict(D=12), E_SIZE), (dict(W=2), E_SIZE), (dict(bits=None), E_NULL),
                 (dict(bits=p.value + 4), E_CONFIG))
    # voxelize
    for kw, st in bad_grids:
        assert vox(grid(**kw), 4, 2, p, p, p, *tail) == st, kw
    assert vox(None, 4, 2, p, p, p, *tail) == E_NULL and vox(grid(), 0, 2, p, p, p, *tail) == E_SIZE and vox(grid(), 4, 0, p, p, p, *tail) == E_SIZE
    assert vox(grid(), 2 ** 30, 2, p, p, p, *tail) == E_SIZE and vox(grid(), 4, 2 ** 30, p, p, p, *tail) == E_SIZE
    for k in range(3):
        a = [p, p, p]
        a[k] = None
        assert vox(grid(), 4, 2, *a, *tail) == E_NULL
        a[k] = at(2)
        assert vox(grid(), 4, 2, *a, *tail) == E_CONFIG
    assert vox(grid(), 4, 2, at(4), p, p, *tail) == E_CONFIG
    # fill
    q = at(1024)
    for kw, st in bad_grids:
        assert fill(grid(**kw), 0, q, None, None, *tail) == st, kw
    assert fill(grid(), 3, q, q, q, *tail) == E_CONFIG and fill(grid(), -1, q, q, q, *tail) == E_CONFIG
    assert fill(grid(), 0, None, None, None, *tail) == E_NULL and fill(grid(), 1, q, None, None, *tail) == E_NULL and fill(grid(), 2, q, None, None, *tail) == E_NULL
    assert fill(grid(), 0, at(1028), None, None, *tail) == E_CONFIG and fill(grid(), 1, q, None, at(1026), *tail) == E_CONFIG
    assert fill(grid(), 0, p, None, None, *tail) == E_CONFIG and fill(grid(), 2, q, p, None, *tail) == E_CONFIG            # the surface's own bits
    # isosurface
    need = cr.lib().hc_cage_iso_scratch_bytes(6)
    for kw, st in bad_grids:
        assert count(grid(**kw), p, need, p, *tail) == st, kw
    assert count(grid(), None, need, p, *tail) == E_NULL and count(grid(), p, need, None, *tail) == E_NULL and count(grid(), at(128), need, p, *tail) == E_CONFIG
    assert count(grid(), p, need, at(4), *tail) == E_CONFIG and count(grid(), p, need - 1, p, *tail) == E_CAPACITY
    iso = lambda **kw: ctypes.byref(I(**{**dict(n_vertices=10, n_faces=20, centre=(ctypes.c_double * 3)(0, 0, 0), scale=(ctypes.c_double * 3)(1, 1, 1),
                                              vertices=p.value, faces=p.value), **kw}))
    assert emit(grid(), None, p, need, *tail) == E_NULL and emit(grid(D=12), iso(), p, need, *tail) == E_SIZE and emit(grid(), iso(), p, need - 1, *tail) == E_CAPACITY
    assert emit(grid(), iso(n_vertices=0), p, need, *tail) == E_SIZE and emit(grid(), iso(n_faces=-1), p, need, *tail) == E_SIZE and emit(grid(), iso(n_faces=2 ** 30), p, need, *tail) == E_SIZE
    assert emit(grid(), iso(vertices=None), p, need, *tail) == E_NULL and emit(grid(), iso(faces=None), p, need, *tail) == E_NULL
    assert emit(grid(), iso(vertices=p.value + 2), p, need, *tail) == E_CONFIG and emit(grid(), iso(faces=p.value + 1), p, need, *tail) == E_CONFIG
    assert emit(grid(), iso(scale=(ctypes.c_double * 3)(1, 0, 1)), p, need, *tail) == E_CONFIG and emit(grid(), iso(centre=(ctypes.c_double * 3)(float("nan"), 0, 1)), p, need, *tail) == E_CONFIG
    # smooth and components
    tables = dict.fromkeys(tr.PLAN_TABLES, p.value)
    plan = lambda **kw: ctypes.byref(P(**{**dict(V=4, F=2, E=5, reserved=0), **tables, **kw}))
    ptrs = dict(x=p.value, work=p.value + 512, normals=p.value + 1024, faces=p.value, csr_offsets=p.value, csr_faces=p.value, out=p.value, status=p.value)
    sm = lambda **kw: ctypes.byref(S(**{**dict(mode=0, iterations=3, lam=0.25, mu=0.0), **ptrs, **kw}))
    assert smooth(None, sm(), *tail) == E_NULL and smooth(plan(), None, *tail) == E_NULL
    for kw in (dict(V=0), dict(F=0), dict(E=0), dict(E=7), dict(V=2 ** 30)):
        assert smooth(plan(**kw), sm(), *tail) == E_SIZE, kw
    for name in ("edge_faces", "vert_offsets", "vert_nbr"):
        assert smooth(plan(**{name: None}), sm(), *tail) == E_NULL and smooth(plan(**{name: p.value + 2}), sm(), *tail) == E_CONFIG, name
    assert smooth(plan(), sm(iterations=0), *tail) == E_SIZE and smooth(plan(), sm(iterations=4097), *tail) == E_SIZE
    assert smooth(plan(), sm(mode=2), *tail) == E_CONFIG and smooth(plan(), sm(lam=float("nan")), *tail) == E_CONFIG and smooth(plan(), sm(mu=float("inf")), *tail) == E_CONFIG
    for name in ("x", "work", "out", "status", "normals", "faces", "csr_offsets", "csr_faces"):
        assert smooth(plan(), sm(**{name: None}), *tail) == E_NULL, name
        assert smooth(plan(), sm(**{name: ptrs[name] + 2}), *tail) == E_CONFIG, name
    assert smooth(plan(), sm(mode=1, normals=None, faces=None, csr_offsets=None, csr_faces=None, x=None), *tail) == E_NULL       # TAUBIN needs none of the four
    assert smooth(plan(), sm(work=p.value), *tail) == E_CONFIG and smooth(plan(), sm(normals=p.value), *tail) == E_CONFIG and smooth(plan(), sm(x=p.value + 4), *tail) == E_CONFIG
    assert parts(None, 0, p, p, *tail) == E_NULL and parts(plan(E=0), 0, p, p, *tail) == E_SIZE and parts(plan(), 2, p, p, *tail) == E_CONFIG
    assert parts(plan(), 0, None, None, *tail) == E_NULL and parts(plan(), 1, p, None, *tail) == E_NULL and parts(plan(), 1, at(2), p, *tail) == E_CONFIG
    assert parts(plan(), 1, p, at(2), *tail) == E_CONFIG and parts(plan(edge_faces=None), 0, p, None, *tail) == E_NULL
    assert not any(buf)
