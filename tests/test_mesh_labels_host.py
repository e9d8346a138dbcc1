"""Part-label transfer without a GPU: the oracle (tests/mesh_labels_ref.py) against the reference's own functions
(tests/golden/mesh_labels_cases.npz, tools/gen_mesh_labels_golden.py); the g++ build of csrc/mesh_labels_math.h -- the text the
kernels run -- against the oracle, with and without the run suppression; the fixed cases of each rule; the
ABI surface and its refusals; the Python layer's ValueErrors.  Everything is integer: every comparison is equality."""
import ctypes
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mesh_labels_ref as mr
from conftest import ROOT

E_NULL, E_SIZE, E_CONFIG = -1, -2, -3            # D3GA_E_* (include/d3ga.h)
FACES = [1, 2, 255, 256, 257, 1000]
SIZES = [(1, 1), (1, 5), (3, 1), (17, 63), (16, 64), (9, 260)]
L = 5


def test_oracle_equals_the_reference_functions(golden):
    z = golden("mesh_labels_cases.npz")
    assert [str(n) for n in z["names"]] == ["grid", "octa", "fins"]
    assert z["sizes"].tolist() == [[23, 31], [16, 64]] and z["rings"].tolist() == [1, 2, 10]
    degrees = {}
    for n in ("grid", "octa", "fins"):
        faces = z[f"{n}_faces"]
        F = len(faces)
        table = mr.face_neighbours(faces)
        assert mr.same_neighbours(table, mr.neighbours_from_pairs(z[f"{n}_adjacency"], F))
        degrees[n] = np.bincount((table >= 0).sum(1), minlength=4).tolist()
        assert np.array_equal(mr.median(table, z[f"{n}_labels"]), z[f"{n}_median"])
        part = z[f"{n}_part_per_face"]
        assert part.shape == (F, 9) and not part[0].any()
        assert np.array_equal(mr.majority(mr.histogram(part, L)), z[f"{n}_majority"])
        assert z[f"{n}_majority"][:3].tolist() == [0, 1, 2]                  # no vote; 1 and 3 tie; 2 and 4 tie
        for r in (1, 2, 10):
            for mask, grown in zip(z[f"{n}_masks"], z[f"{n}_grown{r}"]):
                assert np.array_equal(mr.grow(table, mask, r), grown), (n, r)
        assert (z[f"{n}_grown1"] != z[f"{n}_grown2"]).any() and (z[f"{n}_grown1"] != z[f"{n}_masks"]).any()
        for H, W in ((23, 31), (16, 64)):
            p2f, image = z[f"{n}_{H}x{W}_pix_to_face"], z[f"{n}_{H}x{W}_image"]
            assert p2f.shape == (H, W) and p2f.min() == -1 and p2f.max() == F - 1 and set(image.ravel().tolist()) == {0, 1, 2, 3, 4}
            # Renderer.forward at B = 1: the label of the view's pick, 0 on a face no pixel shows
            want = np.zeros(F, np.int32)
            for f, l in mr.view_pick(p2f, image, F).items():
                want[f] = l
            assert np.array_equal(want, z[f"{n}_{H}x{W}_part"]), (n, H, W)
            hist, flag = mr.vote(p2f[None], image[None], F, L)
            assert flag == 0 and np.array_equal(hist.sum(1), np.isin(np.arange(F), p2f).astype(np.int32))
    assert degrees == {"grid": [0, 2, 18, 40], "octa": [0, 0, 0, 128], "fins": [0, 7, 8, 3]}
    fins = mr.face_neighbours(z["fins_faces"])
    assert sorted(fins[14].tolist()) == [-1, 15, 15] and sorted(fins[15].tolist()) == [-1, 14, 14]      # a pair sharing two edges, twice
    assert 12 not in fins[2:4] and sorted(fins[12].tolist()) == [-1, -1, 13]                              # the edge in three faces gives nothing


@pytest.mark.parametrize("H,W", SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("B", [1, 3])
def test_host_vote_equals_the_oracle(H, W, B):
    for F in FACES:
        p2f, labels = mr.random_fragments(F * 7 + H * 1000 + W + B, B, H, W, F, L)
        want, flag = mr.vote(p2f, labels, F, L)
        assert flag == 0
        sent = {}
        for flags in (0, mr.EVERY_PIXEL):
            got, status, sent[flags] = mr.host_vote(p2f, labels, F, L, flags=flags)
            assert status == 0 and got.dtype == np.int32 and np.array_equal(got, want), (F, flags)
        assert sent[mr.EVERY_PIXEL] == int(((p2f >= 0) & (p2f < F)).sum()) and sent[0] <= sent[mr.EVERY_PIXEL]
        # uint8 labels, a padded pitch, the (B,1,H,W) view; accumulation on top of an earlier histogram
        padded = np.full((B, 1, H + 1, W + 3), 0xEE, np.uint8)
        padded[:, 0, :H, :W] = labels
        got, status, _ = mr.host_vote(p2f, padded[:, :, :H, :W], F, L, hist=want)
        assert status == 0 and np.array_equal(got, 2 * want)
        wide = np.full((B, H, W + 2), -77, np.int32)
        wide[:, :, :W] = labels
        assert np.array_equal(mr.host_vote(p2f, wide[:, :, :W], F, L)[0], want)


@pytest.mark.parametrize("F", FACES)
def test_host_majority_median_and_growth_equal_the_oracle(F):
    rng = np.random.default_rng(F)
    faces = mr.random_mesh(F, F)
    table = mr.face_neighbours(faces)
    assert table.shape == (F, 3)
    hist = rng.integers(0, 4, (F, 7)).astype(np.int32)
    hist[rng.random(F) < 0.2] = 0
    assert np.array_equal(mr.host_majority(hist), mr.majority(hist))
    labels = rng.integers(0, 9, F).astype(np.int32)
    assert np.array_equal(mr.host_median(table, labels), mr.median(table, labels))
    for density in (0.05, 0.5):
        mask = rng.random(F) < density
        for r in (0, 1, 2, 3, 10):
            assert np.array_equal(mr.host_grow(table, mask, r), mr.grow(table, mask, r)), (density, r)


def _vote1(p2f, labels, F, L=L, **kw):
    """one view through the g++ build AND the oracle (they must agree) -> (hist, flag)"""
    p2f, labels = np.asarray(p2f, np.int32)[None], np.asarray(labels, np.int32)[None]
    want, flag = mr.vote(p2f, labels, F, L)
    for flags in (0, mr.EVERY_PIXEL):
        got, status, _ = mr.host_vote(p2f, labels, F, L, flags=flags, **kw)
        assert np.array_equal(got, want) and status == flag
    return want, flag


def test_fixed_cases_of_the_vote():
    # the last pixel in raster order wins, within a row and across rows
    hist, flag = _vote1([[0, 0, 1, 0], [1, -1, -1, -1]], [[1, 2, 3, 4], [2, 0, 0, 0]], 2)
    assert flag == 0 and hist.tolist() == [[0, 0, 0, 0, 1], [0, 0, 1, 0, 0]]
    # a label equal to L - 1 is counted; a background label lands in column 0
    hist, flag = _vote1([[0, 1]], [[L - 1, 0]], 2)
    assert flag == 0 and hist.tolist() == [[0, 0, 0, 0, 1], [1, 0, 0, 0, 0]]
    # a label equal to L and a label of -1 set the flag and count nothing -- but only at a pixel that votes
    for bad in (L, -1):
        hist, flag = _vote1([[0, 1]], [[bad, 2]], 2)
        assert flag == 1 and hist.tolist() == [[0] * L, [0, 0, 1, 0, 0]]
        hist, flag = _vote1([[0, 0, -1]], [[bad, 2, bad]], 1)
        assert flag == 0 and hist.tolist() == [[0, 0, 1, 0, 0]]
    # a pix_to_face >= F is ignored, as is anything below 0
    hist, flag = _vote1([[2, 5, -3, 1]], [[1, 1, 1, 3]], 2)
    assert flag == 0 and hist.tolist() == [[0] * L, [0, 0, 0, 1, 0]]
    # the flag is sticky: a later clean call leaves it set
    p2f, bad, good = np.zeros((1, 1, 4), np.int32), np.full((1, 1, 4), 9, np.int32), np.ones((1, 1, 4), np.int32)
    cells, hist, status = np.zeros((1, 1), np.uint32), np.zeros((1, L), np.int32), np.zeros(1, np.uint32)
    for image in (bad, good):
        assert mr.lib().hc_label_vote(1, 1, L, 1, 4, mr._p(p2f), mr._p(image), 0, 16, 0, mr._p(cells), mr._p(hist), mr._p(status), 0, None) == 0
    assert status[0] == 1 and hist.tolist() == [[0, 1, 0, 0, 0]] and not cells.any()


def test_two_views_of_a_batch_equal_two_single_calls():
    """The departure from the reference at B > 1: every view votes on its own."""
    F = 40
    p2f, labels = mr.random_fragments(5, 2, 16, 24, F, L)
    both, _, _ = mr.host_vote(p2f, labels, F, L)
    first, _, _ = mr.host_vote(p2f[:1], labels[:1], F, L)
    second, _, _ = mr.host_vote(p2f[1:], labels[1:], F, L, hist=first)
    assert np.array_equal(both, second) and np.array_equal(both, mr.vote(p2f, labels, F, L)[0])
    seen_twice = np.isin(np.arange(F), p2f[0]) & np.isin(np.arange(F), p2f[1])
    assert seen_twice.any() and (both.sum(1)[seen_twice] == 2).all()


def test_fixed_cases_of_majority_median_and_growth():
    def both(a, b):
        assert np.array_equal(a, b), (a, b)
        return a.tolist()
    hist = np.array([[9, 0, 2, 2, 0], [5, 0, 0, 0, 0], [0, 1, 0, 0, 3], [0, 0, 0, 0, 0], [7, 1, 1, 1, 1]], np.int32)
    assert both(mr.host_majority(hist), mr.majority(hist)) == [2, 0, 4, 0, 1]          # ties to the smallest label; all zero -> 0; column 0 is not a label
    # a strip of four triangles: the ends have one neighbour, the middle ones two; plus a face on its own
    faces = np.array([[0, 1, 2], [1, 3, 2], [2, 3, 4], [3, 5, 4], [6, 7, 8]])
    table = mr.face_neighbours(faces)
    assert np.sort(table, 1).tolist() == [[-1, -1, 1], [-1, 0, 2], [-1, 1, 3], [-1, -1, 2], [-1, -1, -1]]
    labels = np.array([4, 1, 3, 0, 2], np.int32)
    # one neighbour: its label; two with an odd sum: (4 + 3) // 2 = 3, (1 + 0) // 2 = 0; none: the face keeps its own
    assert both(mr.host_median(table, labels), mr.median(table, labels)) == [1, 3, 0, 3, 2]
    fan = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 1], [1, 3, 2]])                        # a tetrahedron: three neighbours each
    t4 = mr.face_neighbours(fan)
    assert both(mr.host_median(t4, np.array([7, 1, 5, 3], np.int32)), mr.median(t4, [7, 1, 5, 3])) == [3, 5, 3, 5]
    for mask in (np.zeros(5, bool), np.ones(5, bool)):                                  # an empty and a full mask are fixed points
        for r in (1, 3):
            assert both(mr.host_grow(table, mask, r), mr.grow(table, mask, r)) == mask.tolist()
    mask = np.array([1, 0, 0, 0, 0], bool)
    assert both(mr.host_grow(table, mask, 0), mr.grow(table, mask, 0)) == mask.tolist()  # n_rings = 0 returns the mask
    # ring 1: face 1 (neighbours 0, 2: one of two inside) marks both; face 0's only neighbour is outside: it does not qualify
    assert both(mr.host_grow(table, mask, 1), mr.grow(table, mask, 1)) == [1, 0, 1, 0, 0]
    # ... and there it stops, as in the reference: face 1 is now surrounded, and faces 0 and 3 see their whole ring inside or outside
    assert both(mr.host_grow(table, mask, 2), mr.grow(table, mask, 2)) == [1, 0, 1, 0, 0]
    assert both(mr.host_grow(table, mask, 10), mr.grow(table, mask, 10)) == [1, 0, 1, 0, 0]


def test_python_neighbour_table_equals_the_oracle(golden):
    from d3ga_amd import mesh_labels as ml
    z = golden("mesh_labels_cases.npz")
    meshes = [z[f"{n}_faces"] for n in ("grid", "octa", "fins")] + [mr.random_mesh(F, F + 1) for F in FACES]
    for faces in meshes:
        got = ml._table_from_faces("t", ml._faces_array("t", faces))
        assert got.dtype == np.int32 and mr.same_neighbours(got, mr.face_neighbours(faces))
        assert not ((got[:, :-1] < 0) & (got[:, 1:] >= 0)).any()                        # padded at the end
        table = ml.face_neighbours(torch.from_numpy(np.asarray(faces))[None], device="cpu")
        assert table.dtype == torch.int32 and np.array_equal(table.numpy(), got)
        pairs = mr.adjacency_pairs(faces)
        mesh = SimpleNamespace(faces=faces, face_adjacency=pairs)
        assert mr.same_neighbours(ml._neighbours("t", mesh, "cpu").numpy(), got)
        assert np.array_equal(ml._neighbours("t", SimpleNamespace(faces=faces), "cpu").numpy(), got)
        assert isinstance(table, ml.FaceNeighbours) and ml._neighbours("t", table, "cpu") is table
        copy = table.clone().to("cpu")                                                  # the type travels with the tensor
        assert isinstance(copy, ml.FaceNeighbours) and ml._neighbours("t", copy, "cpu") is copy
        if (got < 0).any():                                                             # a plain array is a faces array, never a table
            with pytest.raises(ValueError):
                ml._neighbours("t", got, "cpu")
        assert np.array_equal(ml._neighbours("t", np.asarray(faces), "cpu").numpy(), got)


def test_python_layer_validates_on_the_host():
    from d3ga_amd import _lib
    from d3ga_amd.mesh_labels import LabelTransfer, face_neighbours, grow_mask_region, majority_vote, median_filter_mesh
    faces = mr.random_closed_mesh(20, 1)
    B, H, W = 2, 6, 8
    make = lambda **kw: LabelTransfer(**{**dict(faces=faces, n_labels=5, B=B, H=H, W=W, device="cpu"), **kw})
    lt = make()
    assert lt.counts().shape == (20, 5) and lt.cells.shape == (B, 20) and not lt.cells.any() and lt.scratch.key == (B, 12, 20, H, W)
    p2f, part = torch.zeros(B, H, W, dtype=torch.int32), torch.zeros(B, 1, H, W, dtype=torch.int32)
    table = face_neighbours(faces, device="cpu")
    bad = [
        lambda: make(faces=faces[:, :2]), lambda: make(faces=faces.astype(np.float32)), lambda: make(faces=-faces),
        lambda: make(n_labels=0), lambda: make(n_labels=33), lambda: make(B=0), lambda: make(H=0), lambda: make(W=_lib.MESH_MAX_SIDE + 1),
        lambda: make(n_verts=3),
        lambda: lt.add_fragments(p2f.numpy(), part), lambda: lt.add_fragments(p2f.long(), part), lambda: lt.add_fragments(p2f[:1], part),
        lambda: lt.add_fragments(p2f.transpose(1, 2).contiguous().transpose(1, 2), part),              # column-major
        lambda: lt.add_fragments(p2f, part.numpy()), lambda: lt.add_fragments(p2f, part.float()), lambda: lt.add_fragments(p2f, part.long()),
        lambda: lt.add_fragments(p2f, part[..., :-1]), lambda: lt.add_fragments(p2f, torch.zeros(B, 2, H, W, dtype=torch.int32)),
        lambda: lt.add_fragments(p2f, torch.zeros(B, 1, H, 2 * W, dtype=torch.int32)[..., ::2]),         # elements two apart
        lambda: lt.add_fragments(p2f, part[:1].expand(B, 1, H, W)),                                     # frames overlap
        lambda: lt.add_fragments(p2f, torch.zeros(B, 1, H, W, dtype=torch.uint8, device="meta")),
        lambda: lt.add(object(), torch.zeros(B, 12, 3), part),
        lambda: lt.labels(out=torch.zeros(20)), lambda: lt.labels(out=torch.zeros(19, dtype=torch.int32)),
        lambda: majority_vote(), lambda: majority_vote(np.zeros((3, 2), np.int64), hist=np.zeros((3, 2), np.int32)),
        lambda: majority_vote(np.zeros(3, np.int64)), lambda: majority_vote(np.zeros((3, 2))), lambda: majority_vote(np.full((3, 2), 32)),
        lambda: majority_vote(np.full((3, 2), 4), n_labels=4), lambda: majority_vote(hist=np.zeros((3, 33), np.int32)),
        lambda: median_filter_mesh(table, np.zeros(19, np.int64)), lambda: median_filter_mesh(table, np.zeros(20)),
        lambda: median_filter_mesh("mesh", np.zeros(20, np.int64)), lambda: median_filter_mesh(np.zeros((20, 2), np.int64), np.zeros(20, np.int64)),
        lambda: median_filter_mesh(SimpleNamespace(faces=faces, face_adjacency=np.array([[0, 20]])), np.zeros(20, np.int64)),
        lambda: median_filter_mesh(SimpleNamespace(faces=faces, face_adjacency=np.array([[0, 1]] * 4)), np.zeros(20, np.int64)),
        lambda: grow_mask_region(table, np.zeros(20, np.int64)), lambda: grow_mask_region(table, np.zeros(21, bool)),
        lambda: grow_mask_region(table, np.zeros(20, bool), n_rings=-1), lambda: grow_mask_region(table, np.zeros(20, bool), n_rings=4097),
    ]
    for i, fn in enumerate(bad):
        with pytest.raises(ValueError):
            fn()
            pytest.fail(f"case {i} was accepted")
    # everything fits, but the tensors live on the CPU: no fallback
    pitched = torch.zeros(B, 1, H + 1, W + 3, dtype=torch.uint8)[:, :, :H, :W]
    for fn in (lambda: lt.add_fragments(p2f, part), lambda: lt.add_fragments(p2f, part[:, 0]), lambda: lt.add_fragments(p2f, pitched),
               lambda: lt.labels(), lambda: majority_vote(torch.zeros(3, 2, dtype=torch.int64)), lambda: majority_vote(hist=torch.zeros(3, 5, dtype=torch.int32)),
               lambda: median_filter_mesh(table, torch.zeros(20, dtype=torch.int64)), lambda: grow_mask_region(table, torch.zeros(20, dtype=torch.bool))):
        with pytest.raises(_lib.D3GAError):
            fn()
    # add(): MeshCameras or the pytorch3d shim's cameras reach the rasterizer, which refuses CPU tensors; another image size is an argument error
    import compat_ref as cr
    from d3ga_amd.mesh_render import MeshCameras
    s = cr.scene()
    owner = LabelTransfer(s["faces"], 5, 2, cr.H, cr.W, device="cpu", n_verts=s["verts"].shape[1])
    seg = torch.zeros(2, 1, cr.H, cr.W, dtype=torch.int32)
    with cr.compat_path():
        for cams in (cr.shim_cameras(torch), MeshCameras(s["R"], s["t"], s["K"], (cr.H, cr.W), device="cpu")):
            with pytest.raises(_lib.D3GAError):
                owner.add(cams, torch.from_numpy(s["verts"].copy()), seg)
    with pytest.raises(ValueError):
        owner.add(MeshCameras(s["R"], s["t"], s["K"], (cr.H + 1, cr.W), device="cpu"), torch.from_numpy(s["verts"].copy()), seg)
    if not torch.cuda.is_available():
        for fn in (lambda: majority_vote(np.zeros((3, 2), np.int64)), lambda: median_filter_mesh(faces, np.zeros(20, np.int64)),
                   lambda: grow_mask_region(SimpleNamespace(faces=faces), np.zeros(20, bool))):
            with pytest.raises(_lib.D3GAError):
                fn()
    lt.status[0] = 1
    with pytest.raises(ValueError):
        lt.check()
    lt.hist[3, 2] = 4
    lt.reset()
    lt.check()
    assert not lt.hist.any()


def test_new_abi_surface():
    from d3ga_amd import _lib
    src = open(os.path.join(ROOT, "include", "d3ga.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], capture_output=True, text=True, check=True).stdout
    for name, n_args in (("d3ga_label_vote", 15), ("d3ga_label_majority", 5), ("d3ga_label_median", 5), ("d3ga_label_grow", 7)):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
        assert re.search(r"\bT %s$" % name, out, flags=re.M)                     # through csrc/d3ga.map
        assert len(_lib._SIGNATURES[name][0]) == n_args
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, src).group(1)
        assert decl.count(",") + 1 == n_args
    assert _lib.ABI_VERSION == 112 and re.search(r"#define\s+D3GA_VERSION\s+112\b", src) and _lib.lib().d3ga_version() == 112
    for name, value in (("LABELS_MAX", 32), ("LABEL_RINGS_MAX", 4096), ("LABEL_EVERY_PIXEL", mr.EVERY_PIXEL),
                        ("LABEL_STATUS_RANGE", 1)):
        assert getattr(_lib, name) == value and re.search(r"#define\s+D3GA_%s\s+%d\b" % (name, value), src), name
    assert mr.LABELS_MAX == _lib.LABELS_MAX
    build = open(os.path.join(ROOT, "d3ga_amd", "csrc", "build.py")).read()
    assert "mesh_labels.hip" in build and "mesh_labels_math.h" in build
    import d3ga_amd
    assert d3ga_amd.LabelTransfer and d3ga_amd.face_neighbours and d3ga_amd.majority_vote and d3ga_amd.median_filter_mesh and d3ga_amd.grow_mask_region


def _buffers():
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    return buf, p, ctypes.c_void_p(p.value + 4), ctypes.c_void_p(p.value + 1), ctypes.c_void_p(p.value + 1024)


@pytest.mark.parametrize("which", ["library", "host build"])
def test_vote_entry_point_refuses_bad_arguments_before_any_launch(which):
    """The refusals happen before any HIP call: host buffers stand in for device memory and are never touched.  The g++ build runs
    the same plan function and must give the same statuses."""
    from d3ga_amd import _lib
    buf, p, off4, off1, _ = _buffers()
    H, W = 4, 8
    ok = dict(B=2, F=10, L=5, H=H, W=W, pix_to_face=p, labels=p, label_u8=0, label_pitch=4 * W, label_frame=4 * W * H, cells=p, hist=p, status=p, flags=0)
    if which == "library":
        call = lambda **kw: _lib.lib().d3ga_label_vote(*{**ok, **kw}.values(), None)
    else:
        call = lambda **kw: mr.lib().hc_label_vote(*{**ok, **kw}.values(), None)
    for name in ("B", "F", "L", "H", "W"):
        assert call(**{name: 0}) == E_SIZE and call(**{name: -2}) == E_SIZE, name
    assert call(L=33) == E_SIZE and call(B=65536) == E_SIZE
    big = dict(label_pitch=2 ** 40, label_frame=2 ** 62)
    assert call(H=2 ** 16, W=2 ** 15, **big) == E_SIZE and call(H=262141, W=1, **big) == E_SIZE
    assert call(B=3, F=2 ** 30) == E_SIZE and call(F=2 ** 27, L=32) == E_SIZE
    assert call(label_u8=2) == E_CONFIG and call(label_u8=-1) == E_CONFIG and call(flags=4) == E_CONFIG and call(flags=2) == E_CONFIG and call(flags=-1) == E_CONFIG
    assert call(label_pitch=4 * W - 4) == E_CONFIG and call(label_frame=4 * W * H - 4) == E_CONFIG
    assert call(label_u8=1, label_pitch=W - 1) == E_CONFIG and call(label_u8=1, label_pitch=W, label_frame=W * H - 1) == E_CONFIG
    assert call(label_pitch=4 * W + 2, label_frame=2 ** 20) == E_CONFIG and call(label_frame=4 * W * H + 2) == E_CONFIG
    for name in ("pix_to_face", "labels", "cells", "hist", "status"):
        assert call(**{name: None}) == E_NULL, name
        assert call(**{name: off1}) == E_CONFIG, name
    assert not any(buf)
    if which == "host build":                                 # what is accepted (host memory: only here)
        at = lambda n: ctypes.c_void_p(p.value + n)
        small = dict(B=1, F=1, L=1, H=1, label_frame=0, labels=at(256), cells=at(512), hist=at(768), status=at(1024))
        assert call(**small) == 0 and call(pix_to_face=off4, **small) == 0 and call(flags=mr.EVERY_PIXEL, **small) == 0
        assert call(**{**small, "W": 7}) == 0
        assert call(**{**small, "label_u8": 1, "labels": at(257), "label_pitch": W + 1}) == 0


@pytest.mark.parametrize("which", ["library", "host build"])
def test_face_entry_points_refuse_bad_arguments_before_any_launch(which):
    from d3ga_amd import _lib
    buf, p, off4, off1, q = _buffers()
    r = ctypes.c_void_p(q.value + 1024)
    if which == "library":
        majority = lambda *a: _lib.lib().d3ga_label_majority(*a, None)
        median = lambda *a: _lib.lib().d3ga_label_median(*a, None)
        grow = lambda *a: _lib.lib().d3ga_label_grow(*a, None)
    else:
        majority, median, grow = mr.lib().hc_label_majority, mr.lib().hc_label_median, mr.lib().hc_label_grow
    assert majority(0, 5, p, q) == E_SIZE and majority(4, 0, p, q) == E_SIZE and majority(4, 33, p, q) == E_SIZE and majority(2 ** 27, 32, p, q) == E_SIZE
    assert majority(4, 5, None, q) == E_NULL and majority(4, 5, p, None) == E_NULL
    assert majority(4, 5, off1, q) == E_CONFIG and majority(4, 5, p, off1) == E_CONFIG
    assert median(0, p, q, r) == E_SIZE and median(-1, p, q, r) == E_SIZE and median(2 ** 30, p, q, r) == E_SIZE
    assert median(4, None, q, r) == E_NULL and median(4, p, None, r) == E_NULL and median(4, p, q, None) == E_NULL
    assert median(4, off1, q, r) == E_CONFIG and median(4, p, off1, r) == E_CONFIG and median(4, p, q, off1) == E_CONFIG
    assert median(4, p, q, q) == E_CONFIG                     # in place
    s = ctypes.c_void_p(r.value + 512)
    assert grow(0, 1, p, q, r, s) == E_SIZE and grow(4, -1, p, q, r, s) == E_SIZE and grow(4, 4097, p, q, r, s) == E_SIZE and grow(2 ** 30, 1, p, q, r, s) == E_SIZE
    assert grow(4, 1, None, q, r, s) == E_NULL and grow(4, 1, p, None, r, s) == E_NULL and grow(4, 1, p, q, None, s) == E_NULL
    assert grow(4, 2, p, q, r, None) == E_NULL
    assert grow(4, 1, off1, q, r, s) == E_CONFIG and grow(4, 1, p, q, q, s) == E_CONFIG and grow(4, 2, p, q, r, q) == E_CONFIG and grow(4, 2, p, q, r, r) == E_CONFIG
    at = lambda base, n: ctypes.c_void_p(base.value + n)
    assert grow(4, 1, p, q, at(q, 3), s) == E_CONFIG and grow(4, 1, p, q, at(q, -3), s) == E_CONFIG      # out overlaps mask by one byte
    for bad in (at(q, -7), at(q, 3), at(r, -7), at(r, 3)):                              # a scratch of 8 bytes that touches mask or out anywhere
        assert grow(4, 2, p, q, r, bad) == E_CONFIG
    assert not any(buf)
    if which == "host build":
        table = (ctypes.c_int32 * 12)(*([-1] * 12))
        assert grow(4, 1, table, q, r, None) == 0 and grow(4, 0, table, q, r, None) == 0       # no scratch below two rings
