"""The triangle-mesh rasterizer on the GPU (d3ga_amd/mesh_render.py, csrc/mesh_raster.hip) against the float64 oracle
(tests/mesh_ref.py), at the smallest shapes at which each mechanism can go wrong (mesh_ref.CASES): single triangles of both
windings as face 0 and as face 1 (the mask quirk), two interpenetrating triangles, a triangle larger than the frame (clamped
box, 15 chunks), triangles hanging off the four sides, a 1 x 1 and a 3 x 200 image, faces that must vanish (behind the near
plane, zero area), bumpy spheres from 64 to 20000 faces (sub-pixel triangles, many faces per pixel), B = 3; 53 spheres of
20000 faces (more setup workgroups than one trip of the scan kernel and than two levels of the coverage kernel's search), and
faces that name vertices outside the mesh, given to the raw entry points.

pix_to_face equals the oracle's exactly away from the marginal pixels (|min b| < 1e-4 for some face whose box holds the pixel,
or the two nearest depths within 1e-5 zbuf; at most 2 % of the covered pixels of a case, tests/test_mesh_render_host.py holds
the cases to that); on a marginal pixel the face is one of the oracle's candidates.

Value bars, non-marginal pixels: 8 x the largest deviation of the g++ build of csrc/mesh_raster_math.h (-ffp-contract=off)
from the oracle over all cases, as measured by tests/test_mesh_render_host.py (mesh_ref.MEASURED, mesh_ref.BARS):
                      measured    bar
  bary                1.8e-4      1.44e-3     (the worst: sub-pixel triangles of sphere20000; 4.4e-6 up to 288 faces)
  zbuf, relative      4.1e-6      3.28e-5
  position            4.7e-6      3.76e-5     scene units, the scenes span 1 .. 3
  depth               4.5e-6      3.6e-5      scene units
  shaded colour       7.0e-5      5.6e-4
  normal map          1.3e-7      1.04e-6
  vertex normals      1.3e-7      1.04e-6
The device build has contraction off and correctly rounded division and square root, so it is expected to reproduce the host
build to the bit; the factor 8 is the issue's allowance.
"""
import ctypes

import numpy as np
import pytest
import torch

import mesh_ref as mr

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64                                        # words in front of and behind every output
NAN_BITS = 0x7FC0DEAD                             # a pattern no kernel would produce


def _setup(ref):
    from d3ga_amd import MeshCameras
    c = ref.case
    cam = c["cams"].astype(np.float64)
    K = np.zeros((ref.B, 3, 3))
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = cam[:, 12], cam[:, 13], cam[:, 14], cam[:, 15], 1
    cams = MeshCameras(cam[:, :9].reshape(-1, 3, 3), cam[:, 9:12], K, (ref.H, ref.W))
    assert np.array_equal(cams.data.cpu().numpy(), c["cams"])                 # the oracle and the device read the same 16 floats
    return cams, torch.from_numpy(c["verts"]).to(DEV), torch.from_numpy(c["faces"]).to(DEV)


def _np(*tensors):
    return [t.cpu().numpy() for t in tensors]


def _within(dev):
    for k, v in dev.items():
        assert v <= mr.BARS[k], (k, v, mr.BARS[k])


@pytest.mark.parametrize("name", mr.CASES)
def test_fragments_views_and_maps_against_the_oracle(name):
    from d3ga_amd import Renderer, rasterize_meshes, vertex_normals
    ref = mr.reference(name)
    cams, verts, faces = _setup(ref)
    frag = rasterize_meshes(cams, verts, faces)
    assert frag.pix_to_face.shape == (ref.B, ref.H, ref.W) and frag.pix_to_face.dtype == torch.int32
    assert frag.zbuf.shape == (ref.B, ref.H, ref.W) and frag.bary_coords.shape == (ref.B, ref.H, ref.W, 3)
    pix, zbuf, bary = _np(*frag)
    dev = ref.check_fragments(pix, zbuf, bary)
    rgb = torch.from_numpy(ref.rgb).to(DEV)
    for white in (True, False):
        r = Renderer(white_background=white)
        r.resize(ref.H, ref.W)
        plain, coloured = r.render(cams, verts, faces), r.render(cams, verts, faces, rgb)
        assert plain.shape == (ref.B, ref.H, ref.W, 3)
        dev["image"] = max(dev.get("image", 0.0), ref.check_image(plain.cpu().numpy(), white, False),
                           ref.check_image(coloured.cpu().numpy(), white, True))
        if ref.B == 1:
            one = r(cams, verts, faces.long()[None])                                            # the reference's call: faces (1,F,3) int64
            assert one.shape == (ref.H, ref.W, 3) and torch.equal(one, plain[0]) and torch.equal(r.forward(cams, verts, faces), plain[0])
    pos, nrm, depth, mask = r.maps(cams, verts, faces)
    assert pos.shape == (ref.B, ref.H, ref.W, 3) and depth.shape == (ref.B, ref.H, ref.W, 1) and mask.shape == (ref.B, ref.H, ref.W, 1)
    dev.update(ref.check_maps(*_np(pos, nrm, depth, mask)))
    dev["vertex_normal"] = ref.check_vertex_normals(vertex_normals(verts, faces).cpu().numpy())
    print(f"{name}: " + " ".join(f"{k} {v:.2e}" for k, v in sorted(dev.items())))
    _within(dev)
    if ref.B == 1:
        single = r.map(cams, verts, faces)
        assert [tuple(t.shape) for t in single] == [(ref.H, ref.W, 3), (ref.H, ref.W, 3), (ref.H, ref.W, 1), (ref.H, ref.W, 1)]
        for a, b in zip(single, (pos, nrm, depth, mask)):
            assert torch.equal(a, b[0])
    if name == "tri_face1":                                   # the mask quirk: face 0 is drawn and masked out
        assert (pix == 0).any() and (mask.cpu().numpy()[..., 0][pix == 0] == 0).all() and (mask.cpu().numpy()[..., 0][pix == 1] == 1).all()
    if name == "tri_face0":
        assert (pix == 0).sum() == 147 and (mask == 0).all() and (pos.abs().sum(-1)[frag.pix_to_face == 0] > 0).all()
    if name == "larger_than_frame":
        assert (pix == 0).all()
    if name == "sphere64_plus_dropped":                       # the two added faces vanish: the base mesh's fragments, bit for bit
        base = mr.reference("sphere64")
        c2, v2, f2 = _setup(base)
        other = rasterize_meshes(c2, v2, f2)
        for a, b in zip(frag, other):
            assert torch.equal(a, b)


def test_every_element_of_a_batch_is_its_own_single_call():
    from d3ga_amd import MeshCameras, Renderer, rasterize_meshes
    ref = mr.reference("batch3")
    cams, verts, faces = _setup(ref)
    r = Renderer()
    frag, image, maps = rasterize_meshes(cams, verts, faces), r.render(cams, verts, faces), r.maps(cams, verts, faces)
    frag = [t.clone() for t in frag]
    assert not torch.equal(frag[0][0], frag[0][1])
    for b in range(ref.B):
        row = cams.data[b].double().cpu().numpy()
        K = np.array([[row[12], 0, row[14]], [0, row[13], row[15]], [0, 0, 1]])
        one = MeshCameras(row[:9].reshape(3, 3), row[9:12], K, (ref.H, ref.W))
        assert torch.equal(one.data[0], cams.data[b])
        got = rasterize_meshes(one, verts[b:b + 1], faces)
        for a, w in zip(got, frag):
            assert torch.equal(a[0], w[b])
        assert torch.equal(r(one, verts[b:b + 1], faces), image[b])
        for a, w in zip(r.map(one, verts[b:b + 1], faces), maps):
            assert torch.equal(a, w[b])
        assert ((maps[3][b] == 0) == (frag[0][b] <= 0)[..., None]).all()      # face 0 is masked out in every element


def test_no_faces_and_all_faces_dropped_render_the_background():
    from d3ga_amd import Renderer, rasterize_meshes
    ref = mr.reference("all_dropped")
    cams, verts, faces = _setup(ref)
    for f in (faces, faces[:0], torch.zeros(1, 0, 3, dtype=torch.int64)):
        frag = rasterize_meshes(cams, verts, f)
        assert (frag.pix_to_face == -1).all() and (frag.zbuf == -1).all() and (frag.bary_coords == -1).all()
        assert (Renderer(True).render(cams, verts, f) == 1).all() and (Renderer(False).render(cams, verts, f) == 0).all()
        for t in Renderer().maps(cams, verts, f):
            assert (t == 0).all()


def _all_outputs(r, cams, verts, faces, rgb, **kw):
    from d3ga_amd import vertex_normals
    image = r.render(cams, verts, faces, rgb, **{k: (v[0] if k == "out" else v) for k, v in kw.items()})
    maps = r.maps(cams, verts, faces, **{k: (v[1] if k == "out" else v) for k, v in kw.items()})
    return (image,) + tuple(maps) + (vertex_normals(verts, faces),)


@pytest.mark.parametrize("name", ("sphere288", "sphere20000"))
def test_two_runs_are_bit_identical_and_out_and_scratch_change_nothing(name):
    from d3ga_amd import Renderer, rasterize_meshes
    ref = mr.reference(name)
    cams, verts, faces = _setup(ref)
    rgb = torch.from_numpy(ref.rgb).to(DEV)
    r = Renderer()
    first = _all_outputs(r, cams, verts, faces, rgb) + tuple(t.clone() for t in rasterize_meshes(cams, verts, faces))
    second = _all_outputs(r, cams, verts, faces, rgb) + tuple(rasterize_meshes(cams, verts, faces))
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    scratch = r.scratch(cams, verts, faces)
    out = (torch.empty_like(first[0]), tuple(torch.empty_like(t) for t in first[1:5]))
    for _ in range(2):                                        # the second round meets a used scratch
        got = _all_outputs(r, cams, verts, faces, rgb, out=out, scratch=scratch)
        assert got[0] is out[0] and all(a is b for a, b in zip(got[1:5], out[1]))
        for a, b in zip(got, first):
            assert torch.equal(a, b)
    for a, b in zip(rasterize_meshes(cams, verts, faces, scratch=scratch), first[6:]):
        assert torch.equal(a, b)
    with pytest.raises(ValueError):
        r.render(cams, verts[:, :-1], faces[:1], scratch=scratch)
    with pytest.raises(ValueError):
        r.render(cams, verts, faces, out=out[0][..., :2])


def test_raw_entry_points_stay_inside_their_buffers():
    """Every output between guard bands, every element written; odd sizes, several workgroups."""
    from d3ga_amd import _lib
    from d3ga_amd.mesh_render import MeshTopology
    L = _lib.lib()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    for name in ("batch3", "larger_than_frame", "sphere288"):
        ref = mr.reference(name)
        cams, verts, faces = _setup(ref)
        B, V, F, H, W = ref.B, ref.V, ref.F, ref.H, ref.W
        topo = MeshTopology(faces)
        off, lists = topo.csr(V, DEV)
        n = ctypes.c_size_t()
        assert L.d3ga_mesh_raster_scratch_bytes(B, V, F, H, W, ctypes.byref(n)) == 0
        bufs = {}

        def guarded(key, shape, dtype=torch.float32, words_per=1):
            count = int(np.prod(shape)) * words_per
            raw = torch.full((count + 2 * GUARD,), NAN_BITS, dtype=torch.int32, device=DEV)
            bufs[key] = raw
            return raw[GUARD:GUARD + count].view(dtype).view(shape)

        scratch = guarded("scratch", ((n.value + 3) // 4,), torch.int32)
        pix, zbuf, bary = guarded("pix", (B, H, W), torch.int32), guarded("zbuf", (B, H, W)), guarded("bary", (B, H, W, 3))
        image, normals = guarded("image", (B, H, W, 3)), guarded("normals", (B, V, 3))
        pos, nrm, depth, mask = guarded("pos", (B, H, W, 3)), guarded("nrm", (B, H, W, 3)), guarded("depth", (B, H, W, 1)), guarded("mask", (B, H, W, 1))
        s = _lib.stream_handle()
        bg = (ctypes.c_float * 3)(1, 1, 1)
        assert L.d3ga_mesh_rasterize(B, V, F, H, W, p(verts), p(topo.faces(DEV)), p(cams.data), p(scratch), p(pix), p(zbuf), p(bary), s) == 0
        assert L.d3ga_mesh_shade_flat(B, V, F, H, W, p(verts), p(topo.faces(DEV)), None, p(cams.data), p(pix), p(bary), bg, p(image), s) == 0
        assert L.d3ga_mesh_vertex_normals(B, V, F, p(verts), p(topo.faces(DEV)), p(off), p(lists), p(normals), s) == 0
        assert L.d3ga_mesh_maps(B, V, F, H, W, p(verts), p(topo.faces(DEV)), p(normals), p(cams.data), p(pix), p(bary), p(pos), p(nrm), p(depth),
                                p(mask), s) == 0
        torch.cuda.synchronize()
        for key, raw in bufs.items():
            assert (raw[:GUARD] == NAN_BITS).all() and (raw[-GUARD:] == NAN_BITS).all(), (name, key)
            if key != "scratch":
                assert not (raw[GUARD:-GUARD] == NAN_BITS).any(), (name, key)
        ref.check_fragments(*_np(pix, zbuf, bary))
        # pix_to_face alone: zbuf and bary are optional
        pix2 = guarded("pix2", (B, H, W), torch.int32)
        assert L.d3ga_mesh_rasterize(B, V, F, H, W, p(verts), p(topo.faces(DEV)), p(cams.data), p(scratch), p(pix2), None, None, s) == 0
        torch.cuda.synchronize()
        assert torch.equal(pix2, pix) and (bufs["pix2"][:GUARD] == NAN_BITS).all() and (bufs["pix2"][-GUARD:] == NAN_BITS).all()


def test_calls_do_not_synchronise_with_the_host():
    from d3ga_amd import Renderer
    ref = mr.reference("sphere288")
    cams, verts, faces = _setup(ref)
    r = Renderer()
    r.render(cams, verts, faces)                              # the topology of this faces tensor exists
    r.maps(cams, verts, faces)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        image, maps = r.render(cams, verts, faces), r.maps(cams, verts, faces)
        view = r(cams, verts, faces)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(view, image[0]) and maps[0].shape == (1, ref.H, ref.W, 3)


def test_inputs_that_require_grad_are_detached():
    from d3ga_amd import Renderer
    ref = mr.reference("sphere64")
    cams, verts, faces = _setup(ref)
    leaf = verts.clone().requires_grad_(True)
    image = Renderer().render(cams, leaf, faces)
    assert not image.requires_grad and torch.equal(image, Renderer().render(cams, verts, faces))


def test_captured_render_and_maps_follow_their_vertices():
    from d3ga_amd import Renderer
    ref, other = mr.reference("sphere288"), mr.make_case("sphere288")
    cams, verts, faces = _setup(ref)
    moved = torch.from_numpy(mr.sphere(12, 12, 99)[0]).to(DEV)[None]
    assert moved.shape == verts.shape and other["faces"].shape == tuple(faces.shape)
    r = Renderer()
    eager = [(r.render(cams, v, faces), r.maps(cams, v, faces)) for v in (verts, moved)]
    assert not torch.equal(eager[0][0], eager[1][0])
    slot = verts.clone()
    scratch = r.scratch(cams, slot, faces)
    out = (torch.empty_like(eager[0][0]), tuple(torch.empty_like(t) for t in eager[0][1]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                             # warm-up outside the capture, as torch.cuda.graph asks
        r.render(cams, slot, faces, out=out[0], scratch=scratch)
        r.maps(cams, slot, faces, out=out[1], scratch=scratch)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                             # one linear chain of launches
        r.render(cams, slot, faces, out=out[0], scratch=scratch)
        r.maps(cams, slot, faces, out=out[1], scratch=scratch)
    slot.copy_(moved)                                         # new vertex values, written in place
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], eager[1][0])
    for a, b in zip(out[1], eager[1][1]):
        assert torch.equal(a, b)


def test_batch_of_53_spheres_equals_its_single_calls():
    """53 x 20 000 faces are 4141 setup workgroups: mesh_scan_kernel makes five trips of 1024 (each carries the total of those
    before it) and the 64-ary ballot search of mesh_coverage_kernel takes three levels (4141 -> 65 -> 2 -> 1); sphere20000 alone
    has 79 workgroups, one trip and two levels.  Every element must equal its own single call bit for bit."""
    from d3ga_amd import MeshCameras, Renderer, rasterize_meshes
    from d3ga_amd.mesh_render import MeshTopology
    ref = mr.reference("sphere20000")
    B, H, W = 53, ref.H, ref.W
    assert (B * ref.F + 255) // 256 == 4141 > 4 * 1024 and 4141 > 64 * 64
    dirs = np.random.default_rng(53).standard_normal((B, 3))
    rows = np.stack([ref.case["cams"][0]] + [mr._sphere_cam(H, W, 2.5, d) for d in dirs[1:]])
    cam = rows.astype(np.float64)
    K = np.zeros((B, 3, 3))
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = cam[:, 12], cam[:, 13], cam[:, 14], cam[:, 15], 1
    cams = MeshCameras(cam[:, :9].reshape(-1, 3, 3), cam[:, 9:12], K, (H, W))
    assert np.array_equal(cams.data.cpu().numpy(), rows)
    one_v = torch.from_numpy(ref.case["verts"]).to(DEV)
    verts = one_v.expand(B, -1, -1).contiguous()
    topo = MeshTopology(torch.from_numpy(ref.case["faces"]))
    r = Renderer()
    frag, image, maps = rasterize_meshes(cams, verts, topo), r.render(cams, verts, topo), r.maps(cams, verts, topo)
    frag = [t.clone() for t in frag]
    dev = ref.check_fragments(*[t[:1] for t in _np(*frag)])                   # element 0 is sphere20000 itself
    print("batch of 53, element 0: " + " ".join(f"{k} {v:.2e}" for k, v in sorted(dev.items())))
    _within(dev)
    covered = (frag[0] >= 0).reshape(B, -1).sum(1)
    assert int(covered.min()) > 0.2 * H * W                                    # every camera sees the sphere
    for b in range(B):
        one = MeshCameras(cam[b, :9].reshape(3, 3), cam[b, 9:12], K[b], (H, W))
        assert torch.equal(one.data[0], cams.data[b])
        for a, w in zip(rasterize_meshes(one, one_v, topo), frag):
            assert torch.equal(a[0], w[b]), b
        assert torch.equal(r(one, one_v, topo), image[b]), b
        for a, w in zip(r.map(one, one_v, topo), maps):
            assert torch.equal(a, w[b]), b
    assert len({frag[0][b].cpu().numpy().tobytes() for b in range(B)}) == B    # 53 different views


def test_faces_naming_vertices_outside_the_mesh_are_dropped_on_the_device():
    """The Python layer refuses such faces, so only the raw entry points can reach the kernels' own guard.  Four faces that name
    vertex V, V + 1, -1 and -2 at positions 0, 1, the middle and the end of sphere64's face list must do what zero-area faces in
    their places do: nothing.  The bad indices stay within the guard bands of the vertex buffers (64 words = 21 vertices each
    side), so a guard that did not hold would read the band's pattern, not foreign memory."""
    from d3ga_amd import _lib
    L = _lib.lib()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    ref = mr.reference("sphere64")
    cams, verts, _ = _setup(ref)
    B, V, H, W = 1, ref.V, ref.H, ref.W
    base = ref.case["faces"]
    bad = np.array([[V, 1, 2], [3, V + 1, 4], [5, 6, -1], [-2, 7, 8]], np.int32)
    where = (0, 1, len(base) // 2 + 2, len(base) + 3)                          # positions in the list of F + 4
    F = len(base) + 4
    keep = np.ones(F, bool)
    keep[list(where)] = False
    with_bad, with_zero = np.zeros((F, 3), np.int32), np.zeros((F, 3), np.int32)
    with_bad[keep], with_zero[keep] = base, base
    with_bad[~keep] = bad
    assert where == (0, 1, 34, 67) and ((with_bad < 0) | (with_bad >= V)).sum() == 4 and with_bad.min() == -2 and with_bad.max() == V + 1
    assert 3 * 2 <= GUARD                                                      # the farthest word a broken guard would read: 6 off either end

    def guarded(bufs, key, shape, dtype=torch.float32):
        count = int(np.prod(shape))
        raw = torch.full((count + 2 * GUARD,), NAN_BITS, dtype=torch.int32, device=DEV)
        bufs[key] = raw
        return raw[GUARD:GUARD + count].view(dtype).view(shape)

    # The bands of the vertex buffer hold, word for word, the coordinates of a point half way between the camera and the sphere
    # (as vertices -21 .. -1 and V .. V + 20 would): a guard that did not hold would draw a triangle in front of everything.
    cam = ref.case["cams"][0].astype(np.float64)
    eye = -cam[:9].reshape(3, 3).T @ cam[9:12]
    lure = torch.tensor(0.6 * eye, dtype=torch.float32, device=DEV)
    vraw = lure[(torch.arange(3 * V + 2 * GUARD, device=DEV) - GUARD) % 3].contiguous()
    band = (vraw[:GUARD].clone(), vraw[-GUARD:].clone())
    gv = vraw[GUARD:-GUARD].view(B, V, 3)
    gv.copy_(verts)
    inputs = {}
    normals = guarded(inputs, "normals", (B, V, 3))
    s = _lib.stream_handle()
    # d3ga_mesh_vertex_normals reads faces through a CSR that only valid faces can build: the normals come from the oracle
    normals.copy_(torch.from_numpy(mr.vertex_normals_ref(ref.case["verts"][0], base).astype(np.float32))[None])
    n = ctypes.c_size_t()
    assert L.d3ga_mesh_raster_scratch_bytes(B, V, F, H, W, ctypes.byref(n)) == 0
    bg = (ctypes.c_float * 3)(1, 1, 1)
    results = []
    for faces_np in (with_zero, with_bad):
        faces = torch.from_numpy(faces_np).to(DEV)
        bufs = {}
        scratch = guarded(bufs, "scratch", ((n.value + 3) // 4,), torch.int32)
        pix, zbuf, bary = guarded(bufs, "pix", (B, H, W), torch.int32), guarded(bufs, "zbuf", (B, H, W)), guarded(bufs, "bary", (B, H, W, 3))
        image = guarded(bufs, "image", (B, H, W, 3))
        pos, nrm, depth, mask = (guarded(bufs, k, (B, H, W, c)) for k, c in (("pos", 3), ("nrm", 3), ("depth", 1), ("mask", 1)))
        assert L.d3ga_mesh_rasterize(B, V, F, H, W, p(gv), p(faces), p(cams.data), p(scratch), p(pix), p(zbuf), p(bary), s) == 0
        assert L.d3ga_mesh_shade_flat(B, V, F, H, W, p(gv), p(faces), None, p(cams.data), p(pix), p(bary), bg, p(image), s) == 0
        assert L.d3ga_mesh_maps(B, V, F, H, W, p(gv), p(faces), p(normals), p(cams.data), p(pix), p(bary), p(pos), p(nrm), p(depth), p(mask), s) == 0
        torch.cuda.synchronize()
        for key, raw in list(bufs.items()) + list(inputs.items()):
            assert (raw[:GUARD] == NAN_BITS).all() and (raw[-GUARD:] == NAN_BITS).all(), key
            if key != "scratch":
                assert not (raw[GUARD:-GUARD] == NAN_BITS).any(), key
        results.append((pix, zbuf, bary, image, pos, nrm, depth, mask))
    for key, a, b in zip(("pix", "zbuf", "bary", "image", "pos", "nrm", "depth", "mask"), *results):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), key     # bit for bit
    pix = results[1][0].cpu().numpy()
    assert not np.isin(pix, where).any() and (pix >= 0).sum() > 100
    # the faces in between keep their numbers: the oracle's fragments of sphere64, shifted by the faces inserted before them
    shift = np.cumsum(~keep)[keep]
    want = ref.frag[0]["pix_to_face"]
    m = ~ref.frag[0]["marginal"]
    renumbered = np.where(want >= 0, want + shift[np.maximum(want, 0)], -1)
    assert np.array_equal(pix[0][m], renumbered[m])
    # a fragment list that names the four faces all the same: the shade and map kernels have the guard too
    named = torch.from_numpy(np.resize(np.array(where, np.int32), (B, H, W))).to(DEV)
    bufs = {}
    image, pos, nrm, depth, mask = (guarded(bufs, k, (B, H, W, c)) for k, c in (("image", 3), ("pos", 3), ("nrm", 3), ("depth", 1), ("mask", 1)))
    faces = torch.from_numpy(with_bad).to(DEV)
    bary = torch.full((B, H, W, 3), 1 / 3, device=DEV)
    assert L.d3ga_mesh_shade_flat(B, V, F, H, W, p(gv), p(faces), None, p(cams.data), p(named), p(bary), bg, p(image), s) == 0
    assert L.d3ga_mesh_maps(B, V, F, H, W, p(gv), p(faces), p(normals), p(cams.data), p(named), p(bary), p(pos), p(nrm), p(depth), p(mask), s) == 0
    torch.cuda.synchronize()
    for key, raw in bufs.items():
        assert (raw[:GUARD] == NAN_BITS).all() and (raw[-GUARD:] == NAN_BITS).all(), key
    assert torch.equal(vraw[:GUARD], band[0]) and torch.equal(vraw[-GUARD:], band[1]) and torch.equal(gv, verts)
    assert (image == 1).all() and (pos == 0).all() and (nrm == 0).all() and (depth == 0).all()
    assert torch.equal(mask[..., 0], (named > 0).float())
