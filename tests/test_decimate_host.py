"""Quadric edge-collapse decimation without a GPU: the numpy oracle of the rules against the g++ build of
csrc/decimate_math.h -- the text the kernels run -- bit for bit; first-principles properties of every result; the reason for the
feature as a condition; the Python layer's argument rules; the additive ABI."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import cage_author_ref as ca
import decimate_ref as dr
import template_bind_ref as tr

ROOT = dr.ROOT
HOST_CASES = {name: (v, f, t) for name, v, f, t in dr.host_cases()}
SMALL_CASES = {name: (v, f, t, m) for name, v, f, t, m in dr.small_cases()}
NEW_ENTRY_POINTS = {"d3ga_decimate_scratch_bytes": 2, "d3ga_decimate_quadrics": 3, "d3ga_decimate_candidates": 3, "d3ga_decimate_collapse": 3,
                    "d3ga_decimate_faces": 3}


def closed_and_kept(v, f, out, target):
    """the properties a closed 2-manifold keeps: edge census, Euler characteristic, parts, orientation, the count"""
    ov, of, rounds, status = out
    assert status == 0 and rounds >= 1
    twice, once, _ = ca.edge_census(of)
    assert twice and once
    assert dr.euler(of) == dr.euler(f) and dr.parts(of) == dr.parts(f)
    assert ca.signed_volume(ov, of) > 0
    assert len(of) in (target, target - 1)
    assert ov.dtype == np.float32 and of.dtype == np.int32 and len(np.unique(of)) == len(ov) and np.isfinite(ov).all()


@pytest.mark.parametrize("name", list(HOST_CASES))
@pytest.mark.parametrize("shuffled", [False, True], ids=["as built", "rows permuted and rotated"])
def test_oracle_equals_the_host_build_bit_for_bit(name, shuffled):
    v, f, target = HOST_CASES[name]
    assert len(f) <= 1500
    if shuffled:
        v, f = tr.shuffled(v, f, 3)
    host = dr.host_decimate(v, f, target)
    dr.same_result(dr.decimate(v, f, target), host)
    closed_and_kept(v, f, host, target)


def test_decimating_the_fine_surface_beats_the_coarse_grid():
    """The reason for the feature.  capsule_figure at grid radius 16 decimated to the face count of the same figure at radius 8 is
    nearer to the radius-16 surface -- in the largest and the mean distance of its vertices and face centroids, and in volume --
    than the radius-8 mesh, the alternative without decimation."""
    fine_v, fine_f = ca.capsule_figure(r=16, through_host_build=True)
    coarse_v, coarse_f = ca.capsule_figure(r=8)
    out = dr.host_decimate(fine_v, fine_f, len(coarse_f))
    closed_and_kept(fine_v, fine_f, out, len(coarse_f))
    ours = dr.surface_error(out[0], out[1], fine_v, fine_f)
    theirs = dr.surface_error(coarse_v, coarse_f, fine_v, fine_f)
    print("decimated (max, mean, |dV|):", ours, " coarse grid:", theirs, " rounds:", out[2])
    assert ours[0] < theirs[0] and ours[1] < theirs[1] and ours[2] < theirs[2]


@pytest.mark.parametrize("name", list(SMALL_CASES))
def test_edge_cases_oracle_equals_the_host_build(name):
    v, f, target, max_rounds = SMALL_CASES[name]
    dr.same_result(dr.decimate(v, f, target, max_rounds), dr.host_decimate(v, f, target, max_rounds))


def test_a_tetrahedron_cannot_collapse():
    v, f = tr.tetrahedron()
    ov, of, rounds, status = dr.host_decimate(v, f, 2)
    assert status == dr.STATUS_STUCK and rounds == 1
    assert np.array_equal(of, f) and np.array_equal(ov, v.astype(np.float32))


def test_an_octahedron_becomes_a_tetrahedron():
    v, f = dr.octahedron()
    out = dr.host_decimate(v, f, 4)
    closed_and_kept(v, f, out, 4)
    assert len(out[1]) == 4 and len(out[0]) == 4


def test_a_target_at_or_above_the_count_is_the_identity():
    v, f = dr.icosphere(1)
    for target in (len(f), len(f) + 7):
        ov, of, rounds, status = dr.host_decimate(v, f, target)
        assert rounds == 0 and status == 0 and np.array_equal(of, f) and np.array_equal(ov, v.astype(np.float32))


def test_an_open_grid_keeps_its_boundary():
    v, f = tr.grid(17, 17, jitter=0.1)
    boundary = np.nonzero(tr.plan(f, len(v))["vert_boundary"])[0]
    assert len(boundary) == 64
    for target, stuck in ((300, False), (2, True)):
        ov, of, rounds, status = dr.host_decimate(v, f, target)
        assert (status == dr.STATUS_STUCK) == stuck and (stuck or len(of) in (target, target - 1))
        # every boundary vertex is still there, where it was, and the boundary loop is the same set of edges
        rows = {tuple(r) for r in ov.tolist()}
        assert all(tuple(r) in rows for r in v[boundary].astype(np.float32).tolist())
        assert int(tr.plan(of, len(ov))["edge_boundary"].sum()) == 64
        assert dr.euler(of) == dr.euler(f) == 1
    assert len(of) > 2                                       # the last one: stuck above the target, as far as fixed boundaries allow


def test_lists_longer_than_a_wavefront():
    v, f = tr.bipyramid(70)
    assert tr.plan(f, len(v))["max_valence"] == 70
    closed_and_kept(v, f, dr.host_decimate(v, f, 40), 40)


def test_an_unreferenced_vertex_is_dropped():
    v, f = dr.with_unreferenced(*dr.icosphere(1))
    out = dr.host_decimate(v, f, 40)
    closed_and_kept(v, f, out, 40)
    assert not (out[0] == 9.0).any()
    same = dr.host_decimate(*dr.icosphere(1), 40)
    dr.same_result(out, same)                                # numbering aside, the vertex took no part


def test_the_round_limit_sets_stuck():
    v, f = dr.icosphere(2)
    ov, of, rounds, status = dr.host_decimate(v, f, 60, max_rounds=1)
    assert rounds == 1 and status == dr.STATUS_STUCK and 60 < len(of) < len(f)
    assert ca.edge_census(of)[:2] == (True, True) and dr.euler(of) == 2


def test_a_non_manifold_edge_is_refused():
    v, f = tr.tetrahedron()
    v, f = np.concatenate([v, [[2.0, 2, 2]]]), np.concatenate([f, [[0, 1, 4]]]).astype(np.int32)
    for run in (dr.decimate, dr.host_decimate):
        with pytest.raises(ValueError, match="more than 2 faces"):
            run(v, f, 2)


# ---- the Python layer -------------------------------------------------------------------------------------------------------------------
def test_python_layer_refuses_bad_arguments_before_any_launch():
    import d3ga_amd
    from d3ga_amd import cage_author as A
    v, f = dr.icosphere(1)
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    assert d3ga_amd.decimate is A.decimate and d3ga_amd.Decimated is A.Decimated
    for bad in (None, 0, -3, 2.5, True, "many", 2 ** 31):
        with pytest.raises(ValueError, match="tris_target"):
            A.decimate(tv, tf, tris_target=bad)
    for bad in (0, -1, 1.5, True, d3ga_amd._lib.CAGE_MAX_ITERATIONS + 1):
        with pytest.raises(ValueError, match="max_rounds"):
            A.decimate(tv, tf, tris_target=10, max_rounds=bad)
    with pytest.raises(ValueError, match="vertices and faces"):
        A.decimate(tv, None, tris_target=10)
    with pytest.raises(ValueError, match="expected vertices"):
        A.decimate(tv[:, :2], tf, tris_target=10)
    with pytest.raises(ValueError, match="expected faces"):
        A.decimate(tv, tf[:, :2], tris_target=10)
    with pytest.raises(ValueError, match="float32 or float64"):
        A.decimate(tv.to(torch.float16), tf, tris_target=10)
    with pytest.raises(ValueError, match="int32 or int64"):
        A.decimate(tv, tf.to(torch.int16), tris_target=10)
    with pytest.raises(ValueError, match="faces name vertex"):
        A.decimate(tv, tf + 40, tris_target=10)
    nan = tv.clone()
    nan[3, 1] = float("nan")
    with pytest.raises(ValueError, match="not finite"):
        A.decimate(nan, tf, tris_target=10)
    with pytest.raises(d3ga_amd.D3GAError):                  # CPU tensors: refused, nothing is launched
        A.decimate(tv, tf, tris_target=10)

    class Mesh:
        vertices, faces = tv, tf
    with pytest.raises(d3ga_amd.D3GAError):                  # an object with .vertices and .faces is taken apart first
        A.decimate(Mesh(), tris_target=10)


def test_the_default_still_refuses_a_positive_target():
    from d3ga_amd import cage_author as A
    v, f = (torch.from_numpy(a) for a in dr.icosphere(1))
    for call in (lambda **k: A.simplify(v, f, tris_target=50, **k), lambda **k: A.cage_processor(v, f, cage_tris_target=50, **k)):
        with pytest.raises(NotImplementedError, match="quadric decimation is not built yet"):
            call()
        with pytest.raises(NotImplementedError, match="quadric decimation is not built yet"):
            call(decimation=None)
        with pytest.raises(ValueError, match="decimation must be None or 'quadric'"):
            call(decimation="cubic")
    with pytest.raises(ValueError, match="decimation must be None or 'quadric'"):
        A.simplify(v, f, tris_target=0, decimation="cubic")


def test_check_names_the_count_and_the_target():
    from d3ga_amd import _lib
    from d3ga_amd.cage_author import Decimated
    done = Decimated(torch.zeros((4, 3)), torch.zeros((4, 3), dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 3, 4)
    assert done.check() is done and tuple(done) == (done.vertices, done.faces)
    stuck = Decimated(torch.zeros((4, 3)), torch.zeros((4, 3), dtype=torch.int32), torch.full((1,), _lib.CAGE_STATUS_STUCK, dtype=torch.int32), 1, 2)
    with pytest.raises(ValueError, match=r"stopped at 4 faces after 1 rounds, the target was 2"):
        stuck.check()


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------
def test_the_new_entry_points_are_additive():
    import d3ga_amd
    from d3ga_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "d3ga.h")).read(), flags=re.S)
    assert int(re.search(r"#define\s+D3GA_VERSION\s+(\d+)", header).group(1)) == 112 == _lib.ABI_VERSION
    assert int(re.search(r"#define\s+D3GA_CAGE_STATUS_STUCK\s+(\d+)", header).group(1)) == 8 == _lib.CAGE_STATUS_STUCK == dr.STATUS_STUCK
    exported = subprocess.run(["nm", "-D", "--defined-only", d3ga_amd.library_path()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    for name, n_args in NEW_ENTRY_POINTS.items():
        declared = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header)
        assert declared, name
        assert len(declared.group(1).split(",")) == n_args == len(_lib._SIGNATURES[name][0]), name
        assert name in exported and name in _lib.EXPORTS
    fields = re.search(r"typedef struct d3ga_decimate_desc \{(.*?)\} d3ga_decimate_desc;", header, flags=re.S).group(1)
    names = [n.strip(" *") for decl in fields.split(";") if decl.strip() for n in decl.split(",")]
    names = [n.split()[-1].strip("*") for n in names]
    assert names == [n for n, _ in _lib.DecimateDesc._fields_] == [n for n, _ in dr.DecimateStruct._fields_]
    assert ctypes.sizeof(_lib.DecimateDesc) == ctypes.sizeof(dr.DecimateStruct) == 8 + 12 * 8 + 8 + 2 * 8
    nbytes = ctypes.c_int64()
    assert d3ga_amd.lib().d3ga_decimate_scratch_bytes(1000, ctypes.byref(nbytes)) == 0 and nbytes.value == dr.lib().hc_decimate_scratch_bytes(1000)
    assert d3ga_amd.lib().d3ga_decimate_scratch_bytes(0, ctypes.byref(nbytes)) != 0
