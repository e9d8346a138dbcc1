"""Part-label transfer on the GPU (d3ga_amd/mesh_labels.py, csrc/mesh_labels.hip) against the oracle of tests/mesh_labels_ref.py
(itself held to the reference's own functions and to the g++ build of csrc/mesh_labels_math.h by tests/test_mesh_labels_host.py):
the kernels give its integers with and without the run suppression, for int32 and uint8 label images, padded
pitches and the (B,1,H,W) view; the vote scratch is all zero after every call; outputs sit between guard bands.  Equality only."""
import ctypes

import numpy as np
import pytest
import torch

import mesh_labels_ref as mr
import mesh_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
FACES = [1, 2, 255, 256, 257, 1000]
SIZES = [(1, 1), (1, 5), (3, 1), (17, 63), (16, 64), (9, 260)]
L = 5
GUARD = 64                                        # bytes in front of and behind every output (keeps the 16-byte alignment)
FILL = 0xA5


def _guarded(shape, dtype, zero=False):
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    buf = torch.full((n + 2 * GUARD,), FILL, dtype=torch.uint8, device=DEV)
    view = buf[GUARD:GUARD + n].view(dtype).view(shape)
    if zero:
        view.zero_()
    return buf, view


def _bands_intact(buf):
    return bool((buf[:GUARD] == FILL).all()) and bool((buf[-GUARD:] == FILL).all())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _launch_vote(p2f, labels, F, flags=0, hist=None):
    """The ABI call on device tensors, hist and cells between guard bands -> (hist, status); the cells must come back zero."""
    from d3ga_amd import _lib
    B, H, W = p2f.shape
    hbuf, h = _guarded((F, L), torch.int32, zero=True)
    cbuf, cells = _guarded((B, F), torch.int32, zero=True)
    sbuf, status = _guarded((4,), torch.int32, zero=True)
    if hist is not None:
        h.copy_(_dev(hist))
    part = labels[:, 0] if labels.dim() == 4 else labels
    elem = part.element_size()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(_lib.lib().d3ga_label_vote(B, F, L, H, W, p(p2f), p(part), int(part.dtype == torch.uint8), part.stride(1) * elem if H > 1 else W * elem,
                                          part.stride(0) * elem, p(cells), p(h), p(status), flags, _lib.stream_handle()),
               "d3ga_label_vote")
    torch.cuda.synchronize()
    assert _bands_intact(hbuf) and _bands_intact(cbuf) and _bands_intact(sbuf)
    assert not bool(cells.any()), "the vote scratch must be clean after the call"
    assert status[1:].tolist() == [0, 0, 0]
    return h.cpu().numpy(), int(status[0])


@pytest.mark.parametrize("H,W", SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("B", [1, 3])
def test_vote_kernels_equal_the_oracle(H, W, B):
    for F in FACES:
        p2f, labels = mr.random_fragments(F * 7 + H * 1000 + W + B, B, H, W, F, L)
        want, _ = mr.vote(p2f, labels, F, L)
        t_p2f, t_labels = _dev(p2f), _dev(labels)
        for flags in (0, mr.EVERY_PIXEL):
            got, status = _launch_vote(t_p2f, t_labels, F, flags)
            assert status == 0 and got.dtype == want.dtype and np.array_equal(got, want), (F, flags)
        # uint8 labels in a row-padded (B,1,H+1,W+3) buffer, on top of an earlier histogram
        padded = torch.full((B, 1, H + 1, W + 3), 0xEE, dtype=torch.uint8, device=DEV)
        padded[:, 0, :H, :W] = t_labels.to(torch.uint8)
        got, status = _launch_vote(t_p2f, padded[:, :, :H, :W], F, hist=want)
        assert status == 0 and np.array_equal(got, 2 * want), F
        # a pix_to_face that is only 4-byte aligned
        shifted = torch.empty(B * H * W + 1, dtype=torch.int32, device=DEV)[1:].view(B, H, W).copy_(t_p2f)
        assert np.array_equal(_launch_vote(shifted, t_labels, F)[0], want)


def _owner(faces, B, H, W):
    from d3ga_amd.mesh_labels import LabelTransfer
    return LabelTransfer(faces, L, B, H, W, device=DEV)


def test_label_transfer_accumulates_and_leaves_its_scratch_clean():
    F, B, H, W = 300, 2, 24, 40
    faces = mr.random_closed_mesh(F, 3)
    first, second = mr.random_fragments(1, B, H, W, F, L), mr.random_fragments(2, B, H, W, F, L)
    lt = _owner(faces, B, H, W)
    assert lt.counts().shape == (F, L) and not bool(lt.counts().any()) and not bool(lt.cells.any())
    lt.add_fragments(_dev(first[0]), _dev(first[1])[:, None])                          # (B,1,H,W) int32
    assert not bool(lt.cells.any())
    want1, _ = mr.vote(*first, F, L)
    assert np.array_equal(lt.counts().cpu().numpy(), want1)
    lt.add_fragments(_dev(second[0]), _dev(second[1].astype(np.uint8)))                 # (B,H,W) uint8
    assert not bool(lt.cells.any())
    want2, _ = mr.vote(*second, F, L, hist=want1)
    assert np.array_equal(lt.counts().cpu().numpy(), want2) and (want2 != want1).any()
    fresh = _owner(faces, B, H, W)                                                      # the second call alone, on a fresh owner
    fresh.add_fragments(_dev(second[0]), _dev(second[1]))
    assert np.array_equal(fresh.counts().cpu().numpy(), want2 - want1)
    lt.check()
    table = mr.face_neighbours(faces)
    assert mr.same_neighbours(lt.neighbours.cpu().numpy(), table)                       # the order within a row is free
    voted = mr.majority(want2)
    assert np.array_equal(lt.labels(median=False).cpu().numpy(), voted)
    assert np.array_equal(lt.labels().cpu().numpy(), mr.median(table, voted))
    out = torch.full((F,), -5, dtype=torch.int32, device=DEV)
    assert lt.labels(out=out) is out and np.array_equal(out.cpu().numpy(), mr.median(table, voted))
    lt.reset()
    assert not bool(lt.counts().any()) and not bool(lt.labels().any())


def test_out_of_range_labels_set_the_sticky_flag():
    F, B, H, W = 50, 1, 8, 12
    p2f, labels = mr.random_fragments(4, B, H, W, F, L, bad=0.2)
    want, flag = mr.vote(p2f, labels, F, L)
    assert flag == 1
    lt = _owner(mr.random_closed_mesh(F, 1), B, H, W)
    lt.check()
    lt.add_fragments(_dev(p2f), _dev(labels))
    assert np.array_equal(lt.counts().cpu().numpy(), want)
    with pytest.raises(ValueError):
        lt.check()
    clean = np.clip(labels, 0, L - 1)
    lt.add_fragments(_dev(p2f), _dev(clean))                                             # sticky
    with pytest.raises(ValueError):
        lt.check()
    lt.reset()
    lt.add_fragments(_dev(p2f), _dev(clean))
    lt.check()
    # uint8: 255 is out of range too
    got, status = _launch_vote(_dev(p2f), _dev(np.where(labels < 0, 255, labels).astype(np.uint8)), F)
    assert status == 1 and np.array_equal(got, want)


@pytest.mark.parametrize("F", FACES)
def test_face_kernels_equal_the_oracle(F):
    from d3ga_amd.mesh_labels import face_neighbours, grow_mask_region, majority_vote, median_filter_mesh
    rng = np.random.default_rng(F)
    faces = mr.random_mesh(F, F)
    table = mr.face_neighbours(faces)
    t_table = face_neighbours(faces)
    assert t_table.dtype == torch.int32 and t_table.is_cuda and mr.same_neighbours(t_table.cpu().numpy(), table)
    hist = rng.integers(0, 4, (F, 7)).astype(np.int32)
    hist[rng.random(F) < 0.2] = 0
    got = majority_vote(hist=_dev(hist))
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), mr.majority(hist))
    part = rng.integers(-1, 6, (F, 11))
    assert np.array_equal(majority_vote(part), mr.majority(mr.histogram(np.maximum(part, 0), 6)))
    labels = rng.integers(0, 9, F)
    want = mr.median(table, labels)
    assert np.array_equal(median_filter_mesh(t_table, labels), want)                    # numpy in, numpy out
    got = median_filter_mesh(t_table, _dev(labels))
    assert got.dtype == torch.int64 and got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    for density in (0.05, 0.5):
        mask = rng.random(F) < density
        for r in (0, 1, 2, 3, 10):
            got = grow_mask_region(t_table, _dev(mask), r)
            assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), mr.grow(table, mask, r)), (density, r)


def test_drop_ins_equal_the_reference_functions(golden):
    from types import SimpleNamespace

    from d3ga_amd.mesh_labels import grow_mask_region, majority_vote, median_filter_mesh
    z = golden("mesh_labels_cases.npz")
    for n in ("grid", "octa", "fins"):
        mesh = SimpleNamespace(faces=z[f"{n}_faces"], face_adjacency=z[f"{n}_adjacency"])
        bare = SimpleNamespace(faces=z[f"{n}_faces"])
        got = majority_vote(z[f"{n}_part_per_face"])
        assert isinstance(got, np.ndarray) and np.array_equal(got, z[f"{n}_majority"])
        for m in (mesh, bare, z[f"{n}_faces"]):
            got = median_filter_mesh(m, z[f"{n}_labels"])
            assert isinstance(got, np.ndarray) and np.array_equal(got, z[f"{n}_median"])
        for r in (1, 2, 10):
            for mask, grown in zip(z[f"{n}_masks"], z[f"{n}_grown{r}"]):
                got = grow_mask_region(mesh, mask, n_rings=r)
                assert got.dtype == np.bool_ and np.array_equal(got, grown), (n, r)
                assert np.array_equal(grow_mask_region(bare, mask, r), grown)
        # Renderer.forward at B = 1 followed by a vote of one view: the recorded scatter is the label with the single count
        F = len(mesh.faces)
        for H, W in ((23, 31), (16, 64)):
            lt = _owner(mesh.faces, 1, H, W)
            lt.add_fragments(_dev(z[f"{n}_{H}x{W}_pix_to_face"])[None], _dev(z[f"{n}_{H}x{W}_image"])[None, None])
            hist = lt.counts().cpu().numpy()
            part = z[f"{n}_{H}x{W}_part"]
            seen = np.isin(np.arange(F), z[f"{n}_{H}x{W}_pix_to_face"])
            assert np.array_equal(hist.sum(1), seen.astype(np.int32)) and np.array_equal(hist.argmax(1)[seen], part[seen]) and not part[~seen].any()


def test_growth_on_a_closed_mesh_of_1000_faces():
    from d3ga_amd.mesh_labels import face_neighbours, grow_mask_region
    faces = mr.random_closed_mesh(1000, 9)
    table = mr.face_neighbours(faces)
    assert (table >= 0).all()
    t_table = face_neighbours(faces)
    mask = np.random.default_rng(9).random(1000) < 0.03
    grown = {r: mr.grow(table, mask, r) for r in (1, 2, 10)}
    assert mask.sum() < grown[1].sum() < grown[2].sum() < grown[10].sum()
    for r, want in grown.items():
        assert np.array_equal(grow_mask_region(t_table, mask, r), want), r


def test_end_to_end_transfer_recovers_a_known_labelling():
    from d3ga_amd.mesh_labels import LabelTransfer
    from d3ga_amd.mesh_render import MeshCameras, rasterize_meshes
    H, W = 48, 64
    verts, faces = mesh_ref.sphere(24, 20, 31)
    F = len(faces)
    assert F == 960
    gt = (1 + (np.arange(F) * 7 // 13) % 4).astype(np.int32)
    t_gt, t_verts = _dev(gt), _dev(verts)[None]
    lt = LabelTransfer(faces, L, 1, H, W, device=DEV, n_verts=len(verts))
    seen = torch.zeros(F, dtype=torch.bool, device=DEV)
    for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0.01), (0, -1, 0.01), (0, 0, 1), (0, 0, -1)):
        row = mesh_ref._sphere_cam(H, W, 2.6, d).astype(np.float64)
        K = np.array([[row[12], 0, row[14]], [0, row[13], row[15]], [0, 0, 1]])
        cameras = MeshCameras(row[:9].reshape(3, 3), row[9:12], K, (H, W), device=DEV)
        p2f = rasterize_meshes(cameras, t_verts, faces).pix_to_face                   # its own scratch: the owner's is overwritten by add
        image = torch.where(p2f >= 0, t_gt[p2f.clamp(min=0).long()], torch.zeros_like(p2f))
        seen[p2f[p2f >= 0].long()] = True
        lt.add(cameras, t_verts, image[:, None])
        assert torch.equal(lt.scratch.pix_to_face, p2f)
    lt.check()
    seen = seen.cpu().numpy()
    assert seen.sum() > F // 2
    hist = lt.counts().cpu().numpy()
    assert not hist[:, 0].any() and (hist.sum(1) > 0).tolist() == seen.tolist() and hist.sum(1).max() >= 2
    got = lt.labels(median=False).cpu().numpy()
    assert np.array_equal(got[seen], gt[seen]) and not got[~seen].any()


def test_add_fragments_is_capturable():
    F, B, H, W = 257, 2, 17, 64
    lt = _owner(mr.random_mesh(F, 5), B, H, W)
    cases = [mr.random_fragments(20 + k, B, H, W, F, L) for k in range(3)]
    p2f = torch.full((B, H, W), -1, dtype=torch.int32, device=DEV)
    part = torch.zeros(B, 1, H, W, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lt.add_fragments(p2f, part)                                                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lt.add_fragments(p2f, part)
    lt.reset()
    want = np.zeros((F, L), np.int32)
    for a, b in cases:
        p2f.copy_(_dev(a))
        part.copy_(_dev(b)[:, None])
        graph.replay()
        want, _ = mr.vote(a, b, F, L, hist=want)
        assert np.array_equal(lt.counts().cpu().numpy(), want) and not bool(lt.cells.any())
    eager = _owner(mr.random_mesh(F, 5), B, H, W)
    for a, b in cases:
        eager.add_fragments(_dev(a), _dev(b))
    assert torch.equal(eager.counts(), lt.counts())


def test_add_takes_the_cameras_of_the_pytorch3d_shim():
    """lib/segmentation.py:41-47 builds its cameras with cameras_from_opencv_projection: the same votes as with MeshCameras."""
    import compat_ref as cr
    from d3ga_amd.mesh_labels import LabelTransfer
    from d3ga_amd.mesh_render import MeshCameras
    s = cr.scene()
    verts, part = _dev(s["verts"]), torch.randint(0, L, (2, 1, cr.H, cr.W), dtype=torch.int32, device=DEV)
    direct = LabelTransfer(s["faces"], L, 2, cr.H, cr.W, device=DEV, n_verts=verts.shape[1])
    direct.add(MeshCameras(s["R"], s["t"], s["K"], (cr.H, cr.W), device=DEV), verts, part)
    shim = LabelTransfer(s["faces"], L, 2, cr.H, cr.W, device=DEV, n_verts=verts.shape[1])
    with cr.compat_path():
        shim.add(cr.shim_cameras(torch, DEV), verts, part)
    assert torch.equal(shim.counts(), direct.counts())
    p2f = direct.scratch.pix_to_face.cpu().numpy()
    pairs = sum(len(np.unique(view[view >= 0])) for view in p2f)                        # one vote per (view, face it shows)
    assert pairs > 0 and int(direct.counts().sum()) == pairs
    want, _ = mr.vote(p2f, part[:, 0].cpu().numpy(), 200, L)
    assert np.array_equal(direct.counts().cpu().numpy(), want)

