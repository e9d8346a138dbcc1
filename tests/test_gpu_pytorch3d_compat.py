"""compat/pytorch3d and compat/tinycudann on the GPU: `knn_points` (both methods bit-identical to each other and to the g++ build
of csrc/knn_math.h, and held to the float64 oracle of tests/knn_ref.py), `interpolate_face_attributes`, and the shim against the
library it wraps on two closed 200-face meshes and a 3000-point cloud at 70 x 90 (tests/compat_ref.py).

Bars of the map pipeline (position, view depth, normal maps written with the shim: Meshes -> verts_normals_packed,
transform_points, rasterize, two interpolations) against its float64 evaluation at the same fragments and float32 inputs:
8 x the largest deviation of the float32 host pipeline (tests/test_pytorch3d_compat_host.py::test_map_pipeline_on_the_host):
measured position 9.9e-8, depth 3.1e-7, normal 8.6e-8 -> bars 7.9e-7, 2.5e-6, 6.9e-7.

dists figures: the device returns the bits of the g++ build, whose largest error in units of the bar 4 * 2^-24 d + 2^-149 is
<= 0.65 in every case (0.57 on outside_257x1000, where the plain float32 expression alone sat at 1.03: see the host module's
docstring and knn_dist2 in csrc/knn_math.h)."""
import ctypes

import numpy as np
import pytest
import torch

import compat_ref as cr
import knn_ref as kr

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64                                        # words in front of and behind every output
NAN_BITS = 0x7FC0DEAD                             # a pattern no kernel would produce


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def _guarded(bufs, key, shape, dtype=torch.float32):
    words = int(np.prod(shape)) * (2 if dtype == torch.int64 else 1)
    raw = torch.full((words + 2 * GUARD,), NAN_BITS, dtype=torch.int32, device=DEV)
    bufs[key] = raw
    return raw[GUARD:GUARD + words].view(dtype).view(shape)


def _guards_hold(bufs):
    for key, raw in bufs.items():
        assert (raw[:GUARD] == NAN_BITS).all() and (raw[-GUARD:] == NAN_BITS).all(), key
        assert not (raw[GUARD:-GUARD] == NAN_BITS).any(), key


# ---- knn_points ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", kr.CASES)
def test_knn_points_both_methods_equal_the_host_build_and_the_oracle(name):
    from d3ga_amd import knn_points
    c = kr.case(name)
    p1, p2 = torch.from_numpy(c["p1"].copy()).to(DEV), torch.from_numpy(c["p2"].copy()).to(DEV)
    ex = knn_points(p1, p2, K=c["K"], method="exhaustive")
    gr = knn_points(p1, p2, K=c["K"], method="grid")
    assert ex.knn is None and ex.dists.dtype == torch.float32 and ex.idx.dtype == torch.int64
    assert torch.equal(ex.idx, gr.idx) and np.array_equal(_bits(ex.dists), _bits(gr.dists)), "grid and exhaustive differ"
    hd, hi = kr.host_knn(name, "exhaustive")
    assert np.array_equal(ex.idx.cpu().numpy(), hi) and np.array_equal(_bits(ex.dists), hd.view(np.int32)), "device and g++ build differ"
    marginal, worst = kr.check(name, ex.dists.cpu().numpy(), ex.idx.cpu().numpy())
    print(f"{name}: {marginal} marginal rows, dists at {worst:.3f} x the bar")
    assert worst <= 1.0, f"{name}: dists off by {worst:.3f} x the bar 4 * 2^-24 d + 2^-149"


def test_knn_points_paths_threshold_gather_and_the_existing_yardstick():
    from d3ga_amd import knn_points
    from d3ga_amd.knn import GRID_FROM
    from d3ga_amd.tetra import knn_mean_dist2
    assert GRID_FROM == 2048
    p = torch.from_numpy(kr.case("self3000_K4")["p1"][0].copy()).to(DEV)
    for P2 in (2047, 2048):                                   # "auto" changes path here: the result does not
        cloud = p[None, :P2]
        auto, ex = knn_points(p[None, :500], cloud, K=4), knn_points(p[None, :500], cloud, K=4, method="exhaustive")
        assert torch.equal(auto.idx, ex.idx) and np.array_equal(_bits(auto.dists), _bits(ex.dists)), P2
    full = knn_points(p[None], p[None], K=4, return_nn=True, lengths1=torch.tensor([3000]), lengths2=torch.tensor([3000], device=DEV))
    assert full.knn.shape == (1, 3000, 4, 3) and torch.equal(full.knn[0], p[full.idx[0]])
    # models/cage_net.py:66 against models/mesh_net.py:66: the same three values in another summation order
    mean = full.dists[0, :, 1:].mean(-1)
    want = knn_mean_dist2(p)
    assert float(((mean - want).abs() / want).max()) <= 1e-6
    # positional form of the reference, inputs that require grad are detached, the result carries no graph
    q = p[None].clone().requires_grad_(True)
    out = knn_points(q, q, K=4)
    assert not out.dists.requires_grad and torch.equal(out[0], full.dists) and torch.equal(out[1], full.idx)
    with pytest.raises(ValueError, match="K = 17"):
        knn_points(q, q, K=17)
    with pytest.raises(NotImplementedError, match="norm"):
        knn_points(q, q, K=4, norm=1)
    with pytest.raises(NotImplementedError, match="lengths1"):
        knn_points(q, q, K=4, lengths1=torch.tensor([2999], device=DEV))
    bad = p[None].clone()
    bad[0, 7, 1] = float("inf")
    with pytest.raises(ValueError, match="not finite"):
        knn_points(p[None], bad, K=4, method="grid")
    empty = knn_points(p[None, :0], p[None], K=4)
    assert empty.dists.shape == (1, 0, 4) and empty.idx.shape == (1, 0, 4)


def test_knn_raw_entry_points_stay_inside_their_buffers():
    """Odd sizes, K that is no template size (3 -> 4 slots, 5 -> 8, 9 -> 16), several workgroups; every element written."""
    from d3ga_amd import _lib
    from d3ga_amd.knn import _grid
    L, s = _lib.lib(), _lib.stream_handle()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    c = kr.case("outside_257x1000")
    p1, p2 = torch.from_numpy(c["p1"][0].copy()).to(DEV), torch.from_numpy(c["p2"][0].copy()).to(DEV)
    start, items, origin_h, dims = _grid(p2)
    for K in (3, 5, 9):
        bufs = {}
        d1, i1 = _guarded(bufs, "d1", (257, K)), _guarded(bufs, "i1", (257, K), torch.int64)
        d2, i2 = _guarded(bufs, "d2", (257, K)), _guarded(bufs, "i2", (257, K), torch.int64)
        assert L.d3ga_knn_points(1, 257, 1000, K, p(p1), p(p2), p(d1), p(i1), s) == 0
        assert L.d3ga_knn_points_grid(257, 1000, K, p(p1), p(p2), p(start), p(items), origin_h, dims, p(d2), p(i2), s) == 0
        torch.cuda.synchronize()
        _guards_hold(bufs)
        assert torch.equal(i1, i2) and np.array_equal(_bits(d1), _bits(d2)), K
        true = kr.dist64(c["p1"][0], c["p2"][0])
        order = np.argsort(true, axis=1, kind="stable")[:, :K]
        assert (i1.cpu().numpy() == order).mean() > 0.999 and (np.diff(d1.cpu().numpy(), axis=1) >= 0).all()


# ---- interpolate_face_attributes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 3, 6])
def test_interpolate_face_attributes(D):
    from d3ga_amd import _lib, interpolate_face_attributes
    rng = np.random.default_rng(10 + D)
    N, H, W, F = 2, 33, 47, 23                                # N = 2 packed: indices into 2 F faces; a third of the pixels background
    p2f = rng.integers(0, 2 * F, (N, H, W, 1))
    p2f[rng.uniform(size=p2f.shape) < 0.33] = -1
    bary = rng.dirichlet(np.ones(3), p2f.shape).astype(np.float32)
    attrs = (3 * rng.standard_normal((2 * F, 3, D))).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(DEV)
    got = interpolate_face_attributes(t(p2f), t(bary), t(attrs))
    assert got.shape == (N, H, W, 1, D) and got.dtype == torch.float32
    g = got.cpu().numpy()
    m = p2f >= 0
    assert (g[~m] == 0).all() and 0.2 < (~m).mean() < 0.45
    want = (bary.astype(np.float64)[m][:, :, None] * attrs.astype(np.float64)[p2f[m]]).sum(1)
    bar = 4 * 2.0 ** -23 * float(np.abs(attrs).max())
    print(f"D = {D}: largest deviation {float(np.abs(g[m] - want).max()):.2e}, bar {bar:.2e}")
    assert float(np.abs(g[m] - want).max()) <= bar
    assert np.array_equal(g.view(np.int32), kr.host_interp(p2f, bary, attrs).view(np.int32)), "device and g++ evaluation differ"
    # out=, between guard words; an index past the end writes 0; inputs that require grad are detached
    bufs = {}
    out = _guarded(bufs, "out", (N, H, W, 1, D))
    beyond = t(p2f).clone()
    beyond[0, 0, 0, 0], beyond[1, 2, 3, 0] = 2 * F, 2 ** 40
    res = interpolate_face_attributes(beyond, t(bary), t(attrs).requires_grad_(True), out=out)
    torch.cuda.synchronize()
    _guards_hold(bufs)
    assert res is out and not res.requires_grad and float(res[0, 0, 0, 0].abs().max()) == 0 and float(res[1, 2, 3, 0].abs().max()) == 0
    keep = torch.ones(N, H, W, dtype=torch.bool, device=DEV)
    keep[0, 0, 0] = keep[1, 2, 3] = False
    assert torch.equal(res[keep], got[keep])
    assert _lib.lib().d3ga_interp_face_attrs(0, 2 * F, D, None, None, None, None, _lib.stream_handle()) == 0


# ---- the shim against the library it wraps -----------------------------------------------------------------------------------------------
def _scene():
    from d3ga_amd import MeshCameras
    s = cr.scene()
    verts, faces = torch.from_numpy(s["verts"].copy()).to(DEV), torch.from_numpy(s["faces"].copy()).to(DEV)
    cams = MeshCameras(s["R"], s["t"], s["K"], (cr.H, cr.W), device=DEV)
    return s, verts, faces, cams


def _mesh_renderer(R, white):
    lights = R.PointLights(device="cuda:0", location=((0, 0, 1),), ambient_color=((0.45, 0.45, 0.45),), diffuse_color=((0.35, 0.35, 0.35),),
                           specular_color=((0.05, 0.05, 0.05),))
    settings = R.RasterizationSettings(blur_radius=0.0, faces_per_pixel=1, perspective_correct=True, max_faces_per_bin=262144)
    rasterizer = R.MeshRasterizer(raster_settings=settings)
    renderer = R.MeshRenderer(rasterizer, shader=R.HardFlatShader(device="cuda:0", lights=lights,
                                                                   blend_params=R.BlendParams(background_color=[1, 1, 1] if white else [0, 0, 0])))
    renderer.rasterizer.raster_settings.image_size = (cr.H, cr.W)            # Renderer.resize
    return rasterizer, renderer.cuda()


def test_mesh_rasterizer_and_renderer_equal_the_library():
    from d3ga_amd import Renderer, rasterize_meshes
    s, verts, faces, cams = _scene()
    F = faces.shape[0]
    want = rasterize_meshes(cams, verts, faces)
    with cr.compat_path():
        import pytorch3d
        from pytorch3d import renderer as R
        shim_cams = cr.shim_cameras(torch, DEV)
        rasterizer, renderer = _mesh_renderer(R, True)
        meshes = pytorch3d.structures.Meshes(verts=verts, faces=faces[None])
        frag = rasterizer(meshes, cameras=shim_cams)
        assert frag.dists is None and frag.pix_to_face.shape == (2, cr.H, cr.W, 1) and frag.pix_to_face.dtype == torch.int64
        assert frag.zbuf.shape == (2, cr.H, cr.W, 1) and frag.bary_coords.shape == (2, cr.H, cr.W, 1, 3)
        covered = want.pix_to_face >= 0
        shift = torch.arange(2, device=DEV)[:, None, None] * F
        assert torch.equal(frag.pix_to_face[..., 0], torch.where(covered, want.pix_to_face.long() + shift, want.pix_to_face.long()))
        assert torch.equal(frag.zbuf[..., 0], want.zbuf) and torch.equal(frag.bary_coords[:, :, :, 0], want.bary_coords)
        assert 0.2 < float(covered.float().mean()) < 0.9 and int(frag.pix_to_face[1].max()) >= F
        rgb = torch.rand(1, verts.shape[1], 3, generator=torch.Generator().manual_seed(2)).to(DEV)
        for white in (True, False):
            rasterizer, renderer = _mesh_renderer(R, white)
            for colours in (None, rgb):
                textures = None if colours is None else R.TexturesVertex(verts_features=colours)
                renderer.shader.lights.location = shim_cams.get_world_to_view_transform().inverse().get_matrix().transpose(1, 2)[:, :3, 3]
                image = renderer(pytorch3d.structures.Meshes(verts=verts, faces=faces[None], textures=textures), cameras=shim_cams)
                assert image.shape == (2, cr.H, cr.W, 4)
                assert torch.equal(image[..., :3], Renderer(white_background=white).render(cams, verts, faces, colours))
                assert torch.equal(image[..., 3], covered.float())
        # M = N face lists: equal ones are one topology, unequal ones are refused where the topology is built
        same = pytorch3d.structures.Meshes(verts=verts, faces=faces[None].repeat(2, 1, 1))
        assert torch.equal(rasterizer(same, cameras=shim_cams).pix_to_face, frag.pix_to_face)
        other = faces[None].repeat(2, 1, 1)
        other[1, 5] = other[1, 5].flip(0)
        with pytest.raises(NotImplementedError, match="face lists"):
            rasterizer(pytorch3d.structures.Meshes(verts=verts, faces=other), cameras=shim_cams)
        rasterizer.raster_settings.image_size = (cr.H, cr.W + 1)
        with pytest.raises(NotImplementedError, match="image_size"):
            rasterizer(meshes, cameras=shim_cams)


def test_points_renderer_equals_the_library():
    from d3ga_amd import PCRenderer
    s = cr.scene()
    _, _, _, cams = _scene()
    points = torch.from_numpy(s["points"].copy()).to(DEV)
    with cr.compat_path():
        from pytorch3d import renderer as R
        from pytorch3d.structures import Pointclouds
        shim_cams = cr.shim_cameras(torch, DEV)
        for white in (True, False):
            settings = R.PointsRasterizationSettings(image_size=512, points_per_pixel=5, radius=0.03, bin_size=0)
            rasterizer = R.PointsRasterizer(raster_settings=settings)
            renderer = R.PointsRenderer(rasterizer=rasterizer, compositor=R.AlphaCompositor(background_color=[1, 1, 1] if white else [0, 0, 0])).cuda()
            rasterizer.raster_settings.image_size = (cr.H, cr.W)               # PCRenderer.resize
            colours = torch.tensor([[154, 205, 50]]).expand(3000, -1).to(DEV)[None] / 255.0      # recorder/pc_renderer.py:64
            image = renderer(Pointclouds(points=points, features=colours), cameras=shim_cams)
            want = PCRenderer(white_background=white, radius=0.03, points_per_pixel=5).render(cams, points, colours)
            assert image.shape == (2, cr.H, cr.W, 3) and torch.equal(image, want)
            background = 1.0 if white else 0.0
            assert 0.05 < float((image != background).any(-1).float().mean()) < 0.95
            assert torch.equal(renderer(Pointclouds(points=points), cameras=shim_cams),
                               PCRenderer(white_background=white, radius=0.03, points_per_pixel=5).render(cams, points))
        settings.points_per_pixel = 9
        with pytest.raises(ValueError, match="points_per_pixel"):
            renderer(Pointclouds(points=points), cameras=shim_cams)


def test_map_pipeline_written_with_the_shim():
    """recorder/mesh_renderer.py:69-100 in this test's own words, on both meshes at once."""
    from d3ga_amd import Renderer
    s, verts, faces, cams = _scene()
    with cr.compat_path():
        import pytorch3d
        from pytorch3d import renderer as R
        from pytorch3d.ops.interp_face_attrs import interpolate_face_attributes
        shim_cams = cr.shim_cameras(torch, DEV)
        rasterizer, _ = _mesh_renderer(R, True)
        meshes = pytorch3d.structures.Meshes(verts=verts, faces=faces[None])
        packed_faces = meshes.faces_packed()
        position = meshes.verts_packed()
        view = shim_cams.get_world_to_view_transform().transform_points(meshes.verts_padded()).reshape(-1, 3)
        normals = meshes.verts_normals_packed()
        fragments = rasterizer(meshes, cameras=shim_cams)
        mask = (fragments.pix_to_face > 0).float()[..., 0:1]
        maps = interpolate_face_attributes(fragments.pix_to_face, fragments.bary_coords,
                                           torch.cat([position[packed_faces], view[packed_faces]], dim=-1))
        summed = interpolate_face_attributes(fragments.pix_to_face, torch.ones_like(fragments.bary_coords), normals[packed_faces])[:, :, :, 0]
        normal_map = summed / torch.norm(summed, dim=-1, keepdim=True).clamp(min=1e-8)
    p2f, bary = fragments.pix_to_face[..., 0].cpu().numpy(), fragments.bary_coords[:, :, :, 0].cpu().numpy()
    want = cr.maps64(s["verts"], s["faces"], s["R"], s["t"], cr.normals64(), p2f, bary)
    dev = cr.deviations(maps[:, :, :, 0, 0:3].cpu().numpy(), maps[:, :, :, 0, 5].cpu().numpy(), normal_map.cpu().numpy(), want)
    print("shim map pipeline: " + " ".join(f"{k} {v:.2e} (bar {cr.BARS[k]:.2e})" for k, v in sorted(dev.items())))
    for k, v in dev.items():
        assert v <= cr.BARS[k], (k, v)
    bg = torch.from_numpy(p2f < 0).to(DEV)
    assert float(maps[:, :, :, 0][bg].abs().max()) == 0 and float(normal_map[bg].abs().max()) == 0
    # the library's own maps: the same mask per mesh, exactly (mesh 0 loses face 0, as the reference does)
    lib_pos, lib_nrm, lib_depth, lib_mask = Renderer().maps(cams, verts, faces)
    assert torch.equal(mask[0], lib_mask[0])
    assert torch.equal(mask[1], lib_mask[1] + (fragments.pix_to_face[1] == faces.shape[0]).float())       # packed: mesh 1 keeps ITS face 0


# ---- tinycudann -----------------------------------------------------------------------------------------------------------------------
def test_tinycudann_encoding_is_the_sh4_direction_encoding():
    from d3ga_amd.mlp import sh4_direction_encoding
    from compat_ref import COMPOSITE, SH4
    d = torch.rand(1000, 3, generator=torch.Generator().manual_seed(4)).to(DEV)
    g = torch.randn(1000, 16, generator=torch.Generator().manual_seed(5)).to(DEV)
    a = d.clone().requires_grad_(True)
    want = sh4_direction_encoding(a)
    (want * g).sum().backward()
    with cr.compat_path():
        import tinycudann as tcnn
        for cfg in (SH4, COMPOSITE):
            enc = tcnn.Encoding(n_input_dims=3, encoding_config=cfg).cuda()
            b = d.clone().requires_grad_(True)
            out = enc(b)
            assert out.dtype == torch.float32 and out.shape == (1000, 16) and np.array_equal(_bits(out), _bits(want))
            (out * g).sum().backward()
            assert np.array_equal(_bits(b.grad), _bits(a.grad))
