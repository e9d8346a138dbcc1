"""compat/pytorch3d and compat/tinycudann without a GPU: every import statement of the reference that names them resolves
(INTEGRATION.md sec. 1), `matrix_to_quaternion`, the cameras on CPU tensors, the PLY files, and the g++ build of csrc/knn_math.h
(tests/hostcheck/knncheck.cpp) against the float64 brute force of tests/knn_ref.py, on the cases the GPU tests run.

dists figures (the largest error in units of the bar 4 * 2^-24 d + 2^-149, against the float64 distance; the device returns
the same bits): <= 0.65 in every case (0.57 on outside_257x1000); the arithmetic allows 0.75.  The plain float32 expression
`dx*dx + dy*dy + dz*dz` alone sat at 1.03 on 2 of the 257 rows of outside_257x1000: for a query outside p2's box the float32
subtractions q - p round too (coordinates of different binades), which the bar's budget of three products and two additions
does not hold.  knn_dist2 therefore adds the first-order term of what the subtractions lost (csrc/knn_math.h)."""
import io
import math
import os

import numpy as np
import pytest
import torch

import compat_ref as cr
import knn_ref as kr
from conftest import ROOT

# (reference file:line, statement): every import of the reference that names pytorch3d or tinycudann
IMPORTS = (
    ("models/cage_net.py:21", "from pytorch3d.ops import knn_points"),
    ("models/garment_net.py:11", "import pytorch3d"),
    ("models/mesh_net.py:23", "import pytorch3d"),
    ("lib/cage.py:18", "from pytorch3d.transforms import matrix_to_quaternion"),
    ("lib/batch.py:18", "from pytorch3d.transforms import matrix_to_quaternion"),
    ("lib/segmentation.py:21", "from pytorch3d.utils import cameras_from_opencv_projection"),
    ("lib/segmentation.py:22", "from pytorch3d.structures import Meshes"),
    ("lib/segmentation.py:23", "from pytorch3d.renderer import RasterizationSettings, MeshRasterizer, PerspectiveCameras"),
    ("recorder/mesh_renderer.py:7", "import pytorch3d"),
    ("recorder/mesh_renderer.py:11", "from pytorch3d.ops.interp_face_attrs import interpolate_face_attributes"),
    ("recorder/mesh_renderer.py:12-21", "from pytorch3d.renderer import (\n    RasterizationSettings,\n    MeshRenderer,\n    MeshRasterizer,\n"
     "    HardFlatShader,\n    TexturesVertex,\n    PointLights,\n    PerspectiveCameras,\n    BlendParams,\n)"),
    ("recorder/pc_renderer.py:10", "from pytorch3d.utils import cameras_from_opencv_projection"),
    ("recorder/pc_renderer.py:11", "from pytorch3d.structures import Pointclouds"),
    ("recorder/pc_renderer.py:12-18", "from pytorch3d.renderer import (\n    PointsRasterizationSettings,\n    PointsRasterizer,\n"
     "    PerspectiveCameras,\n    PointsRenderer,\n    AlphaCompositor,\n)"),
    ("recorder/pc_renderer.py:19", "from pytorch3d.common.compat import meshgrid_ij"),
    ("utils/graphics_utils.py:13", "from pytorch3d.ops.points_normals import estimate_pointcloud_normals"),
    ("datasets/goliath_dataset.py:28", "from pytorch3d.io import load_ply, save_ply"),
    ("models/mlp.py:13", "import tinycudann as tcnn"),
)
SH4, COMPOSITE = cr.SH4, cr.COMPOSITE


def test_every_import_statement_of_the_reference_resolves_against_compat():
    with cr.compat_path():
        for where, statement in IMPORTS:
            ns = {}
            exec(statement, ns)
            assert len(ns) > 1, where
        import d3ga_amd
        ns = {}
        exec("from pytorch3d.ops import knn_points, interpolate_face_attributes", ns)
        assert ns["knn_points"] is d3ga_amd.knn_points and ns["interpolate_face_attributes"] is d3ga_amd.interpolate_face_attributes
        ns = {}
        exec("import pytorch3d", ns)                                           # a bare import reaches the submodules as attributes
        p3d = ns["pytorch3d"]
        assert os.path.dirname(os.path.dirname(p3d.__file__)) == cr.COMPAT
        for sub in ("structures", "transforms", "ops", "renderer", "utils", "io", "common"):
            assert hasattr(p3d, sub), sub
        assert callable(p3d.structures.Meshes) and callable(p3d.transforms.matrix_to_quaternion)      # recorder/mesh_renderer.py:61, models/garment_net.py:187
        assert p3d.ops.interp_face_attrs.interpolate_face_attributes is d3ga_amd.interpolate_face_attributes
        with pytest.raises(NotImplementedError, match="estimate_pointcloud_normals"):
            p3d.ops.points_normals.estimate_pointcloud_normals(torch.zeros(1, 8, 3))
        a, b = p3d.common.compat.meshgrid_ij(torch.arange(2), torch.arange(3))
        assert a.shape == (2, 3) and a[1, 0] == 1 and b[0, 2] == 2
        # the wrappers of the reference construct without a GPU, and .cuda() on them would pass through: parameter-free modules
        R = p3d.renderer
        lights = R.PointLights(device="cuda:0", location=((0, 0, 1),), ambient_color=((0.45, 0.45, 0.45),), diffuse_color=((0.35, 0.35, 0.35),),
                               specular_color=((0.05, 0.05, 0.05),))
        settings = R.RasterizationSettings(blur_radius=0.0, faces_per_pixel=1, perspective_correct=True, max_faces_per_bin=262144)
        rasterizer = R.MeshRasterizer(raster_settings=settings)
        renderer = R.MeshRenderer(rasterizer, shader=R.HardFlatShader(device="cuda:0", lights=lights, blend_params=R.BlendParams(background_color=[1, 1, 1])))
        renderer.rasterizer.raster_settings.image_size = (7, 9)
        renderer.shader.lights.location = torch.zeros(1, 3)
        assert rasterizer.raster_settings.image_size == (7, 9) and not list(renderer.parameters()) and isinstance(renderer, torch.nn.Module)
        pcs = R.PointsRasterizationSettings(image_size=512, points_per_pixel=5, radius=0.007, bin_size=0)
        points = R.PointsRenderer(rasterizer=R.PointsRasterizer(raster_settings=pcs), compositor=R.AlphaCompositor(background_color=[0, 0, 0]))
        assert not list(points.parameters()) and points.compositor.white_background is False
        with pytest.raises(NotImplementedError, match="ambient_color"):
            R.PointLights()
        with pytest.raises(NotImplementedError, match="background_color"):
            R.BlendParams(background_color=[0.5, 0.5, 0.5])
        with pytest.raises(NotImplementedError, match="blur_radius"):
            R.RasterizationSettings(blur_radius=1e-3)._check()
        with pytest.raises(NotImplementedError, match="faces_per_pixel"):
            R.RasterizationSettings(faces_per_pixel=2)._check()
        with pytest.raises(NotImplementedError):
            R.PerspectiveCameras(focal_length=1.0)
        with pytest.raises(NotImplementedError, match="lists"):
            p3d.structures.Meshes(verts=[torch.zeros(3, 3)], faces=[torch.zeros(1, 3, dtype=torch.int64)])
        m = p3d.structures.Meshes(verts=torch.zeros(2, 4, 3), faces=torch.tensor([[[0, 1, 2], [1, 2, 3]]]))
        assert m.verts_packed().shape == (8, 3) and m.verts_padded().shape == (2, 4, 3) and len(m) == 2
        assert m.faces_packed().tolist() == [[0, 1, 2], [1, 2, 3], [4, 5, 6], [5, 6, 7]] and m.faces_packed().dtype == torch.int64
        # tinycudann
        tcnn = __import__("tinycudann")
        for cfg in (SH4, COMPOSITE):
            enc = tcnn.Encoding(n_input_dims=3, encoding_config=cfg)
            assert enc.n_output_dims == 16 and not list(enc.parameters())
        for cfg in ({"otype": "SphericalHarmonics", "degree": 3}, {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2}):
            with pytest.raises(NotImplementedError, match="encoding_config"):
                tcnn.Encoding(n_input_dims=3, encoding_config=cfg)
        with pytest.raises(NotImplementedError):
            tcnn.Encoding(n_input_dims=2, encoding_config=SH4)
    import sys
    assert cr.COMPAT not in sys.path and "pytorch3d" not in sys.modules and "tinycudann" not in sys.modules


# ---- matrix_to_quaternion ---------------------------------------------------------------------------------------------------
def _m2q():
    with cr.compat_path():
        from pytorch3d.transforms import matrix_to_quaternion
    return matrix_to_quaternion


def _q2m(q):
    r, i, j, k = torch.unbind(q, -1)
    two = 2.0 / (q * q).sum(-1)
    return torch.stack([1 - two * (j * j + k * k), two * (i * j - k * r), two * (i * k + j * r),
                        two * (i * j + k * r), 1 - two * (i * i + k * k), two * (j * k - i * r),
                        two * (i * k - j * r), two * (j * k + i * r), 1 - two * (i * i + j * j)], -1).reshape(q.shape[:-1] + (3, 3))


def _random_rotations(n, dtype, seed=0):
    q = torch.randn(n, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))
    return _q2m(q / q.norm(dim=-1, keepdim=True)).to(dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_matrix_to_quaternion(dtype):
    m2q = _m2q()
    bar = 16 * (2.0 ** -52 if dtype == torch.float64 else 2.0 ** -23)       # 16 ulp of 1: the chosen q_abs is >= 1, nothing is amplified
    known = {                                                                # the identity and the half turns: one per diagonal branch
        (1.0, 1.0, 1.0): (1.0, 0.0, 0.0, 0.0), (1.0, -1.0, -1.0): (0.0, 1.0, 0.0, 0.0),
        (-1.0, 1.0, -1.0): (0.0, 0.0, 1.0, 0.0), (-1.0, -1.0, 1.0): (0.0, 0.0, 0.0, 1.0)}
    for diag, want in known.items():
        q = m2q(torch.diag(torch.tensor(diag, dtype=dtype)))
        assert q.shape == (4,) and q.dtype == dtype and float((q - torch.tensor(want, dtype=dtype)).abs().max()) <= bar, (diag, q)
    h = math.sqrt(0.5)
    quarter = {"x": ([[1, 0, 0], [0, 0, -1], [0, 1, 0]], (h, h, 0, 0)), "y": ([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], (h, 0, h, 0)),
               "z": ([[0, -1, 0], [1, 0, 0], [0, 0, 1]], (h, 0, 0, h))}
    for axis, (m, want) in quarter.items():
        q = m2q(torch.tensor(m, dtype=dtype))
        assert float((q - torch.tensor(want, dtype=dtype)).abs().max()) <= bar, axis
        q = m2q(torch.tensor(m, dtype=dtype).T)                              # the quarter turn back: the real part stays >= 0
        assert float((q - torch.tensor(want, dtype=dtype) * torch.tensor([1, -1, -1, -1], dtype=dtype)).abs().max()) <= bar, axis
    R = _random_rotations(1000, dtype)
    q = m2q(R)
    assert q.shape == (1000, 4) and (q[:, 0] >= 0).all()
    worst = float((_q2m(q.double()) - R.double()).abs().max())
    norm = float(((q.double() ** 2).sum(-1) - 1).abs().max())
    print(f"{dtype}: round trip {worst:.2e}, |q|^2 - 1 {norm:.2e}, bar {bar:.2e}")
    assert worst <= bar and norm <= bar
    assert m2q(R.reshape(10, 100, 3, 3)).shape == (10, 100, 4)
    with pytest.raises(ValueError):
        m2q(torch.zeros(3, 4))


def test_matrix_to_quaternion_gradients():
    m2q = _m2q()
    R = _random_rotations(6, torch.float64, seed=3).requires_grad_(True)
    assert torch.autograd.gradcheck(m2q, (R,), eps=1e-6, atol=1e-6)


# ---- cameras on CPU tensors ----------------------------------------------------------------------------------------------------
def test_cameras_work_on_cpu_tensors():
    s = cr.scene()
    with cr.compat_path():
        cams = cr.shim_cameras(torch)
        assert len(cams) == 2 and cams.image_hw() == (cr.H, cr.W) and not cams._mesh_cameras.keys() - {"hw"}
        R, t = torch.from_numpy(s["R"].copy()).double(), torch.from_numpy(s["t"].copy()).double()
        centre = -(R.transpose(1, 2) @ t[..., None])[..., 0]                                    # -R^T t
        tf = cams.get_world_to_view_transform()
        got = tf.inverse().get_matrix().transpose(1, 2)[:, :3, 3]                              # recorder/mesh_renderer.py:63
        assert got.shape == (2, 3) and float((got.double() - centre).abs().max()) <= 1e-5
        axis = R[:, 2]                                                                          # the optical axis in world space
        on_axis = (centre + 1.7 * axis).float()[:, None, :]                                     # (2,1,3)
        v = tf.transform_points(on_axis)
        assert v.shape == (2, 1, 3) and float((v[:, 0] - torch.tensor([0.0, 0.0, 1.7])).abs().max()) <= 1e-5
        right = (centre + 1.7 * axis + 0.25 * R[:, 0]).float()[:, None, :]                      # OpenCV +x (right) is view -x (left is +x)
        v = tf.transform_points(right)
        assert float((v[:, 0] - torch.tensor([-0.25, 0.0, 1.7])).abs().max()) <= 1e-5
        down = (centre + 1.7 * axis + 0.25 * R[:, 1]).float()[:, None, :]
        assert float((tf.transform_points(down)[:, 0] - torch.tensor([0.0, -0.25, 1.7])).abs().max()) <= 1e-5
        one = cr.shim_cameras(torch, n=1).get_world_to_view_transform()
        packed = torch.from_numpy(s["verts"][0].copy())
        assert one.transform_points(packed).shape == packed.shape                              # (V,3) as recorder/mesh_renderer.py:73 passes it
        M = tf.get_matrix()
        assert M.shape == (2, 4, 4) and torch.equal(M[:, :3, 3], torch.zeros(2, 3)) and torch.equal(M[:, 3, 3], torch.ones(2))
        assert torch.equal(M[:, 3, :3], torch.from_numpy(s["t"].copy()) * torch.tensor([-1.0, -1.0, 1.0]))
        with pytest.raises(ValueError):
            from pytorch3d.utils import cameras_from_opencv_projection
            cameras_from_opencv_projection(torch.zeros(3, 3), torch.zeros(1, 3), torch.zeros(1, 3, 3), torch.zeros(1, 2))


# ---- PLY ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ascii", [False, True])
def test_ply_round_trips(tmp_path, ascii):
    with cr.compat_path():
        from pytorch3d.io import load_ply, save_ply
    verts, faces = cr.closed_sphere()
    path = str(tmp_path / "mesh.ply")
    save_ply(path, torch.from_numpy(verts), torch.from_numpy(faces), ascii=ascii)
    v, f = load_ply(path)
    assert v.dtype == torch.float32 and f.dtype == torch.int64 and np.array_equal(v.numpy(), verts) and np.array_equal(f.numpy(), faces)
    buf = io.BytesIO()
    save_ply(buf, verts, faces, ascii=ascii)
    v, f = load_ply(io.BytesIO(buf.getvalue()))                               # datasets/goliath_dataset.py:268,385
    assert np.array_equal(v.numpy(), verts) and np.array_equal(f.numpy(), faces)
    assert open(path, "rb").read() == buf.getvalue()
    buf = io.BytesIO()
    save_ply(buf, verts, ascii=ascii)                                         # no face element
    v, f = load_ply(io.BytesIO(buf.getvalue()))
    assert np.array_equal(v.numpy(), verts) and f.shape == (0, 3) and f.dtype == torch.int64


def test_ply_reads_other_writers_files_and_refuses_the_rest():
    with cr.compat_path():
        from pytorch3d.io import load_ply
    text = ("ply\nformat ascii 1.0\ncomment made by hand\nelement vertex 4\nproperty double x\nproperty double y\nproperty double z\n"
            "property uchar red\nelement face 2\nproperty list uchar uint vertex_index\nend_header\n"
            "0 0 0 255\n1 0 0 0\n0 1 0 7\n0 0 1.5 9\n3 0 1 2\n3 0 2 3\n")
    v, f = load_ply(io.BytesIO(text.encode()))
    assert v.tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1.5]] and f.tolist() == [[0, 1, 2], [0, 2, 3]]
    head = b"ply\nformat binary_little_endian 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\nproperty short q\nend_header\n"
    rec = np.zeros(2, np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("q", "<i2")]))
    rec["x"], rec["z"], rec["q"] = [1, 2], [5, 6], [-3, 3]
    v, f = load_ply(io.BytesIO(head + rec.tobytes()))
    assert v.tolist() == [[1, 0, 5], [2, 0, 6]] and f.shape == (0, 3)
    with pytest.raises(NotImplementedError, match="triangles"):
        load_ply(io.BytesIO(text.replace("3 0 2 3", "4 0 1 2 3").encode()))
    with pytest.raises(NotImplementedError, match="format"):
        load_ply(io.BytesIO(text.replace("ascii", "binary_big_endian").encode()))
    with pytest.raises(ValueError):
        load_ply(io.BytesIO(b"not a ply"))


# ---- knn_math.h under g++ ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", kr.CASES)
def test_host_build_of_knn_equals_the_oracle(name):
    ref = kr.oracle(name)
    rows = ref["marginal"].size
    share = float(ref["marginal"].sum()) / rows
    dists, idx = kr.host_knn(name, "exhaustive")
    gd, gi = kr.host_knn(name, "grid")
    assert np.array_equal(dists.view(np.int32), gd.view(np.int32)) and np.array_equal(idx, gi), "the ring search differs from the exhaustive one"
    marginal, worst = kr.check(name, dists, idx)
    print(f"{name}: {marginal} of {rows} rows marginal ({share * 100:.2f} %), dists at {worst:.3f} x the bar")
    assert share <= kr.MARGINAL_CAP
    c = kr.case(name)
    if name == "twice200":                                    # both copies of a point list the lower index first, at distance 0
        assert np.array_equal(idx[0, :, 0], np.arange(400) % 200) and np.array_equal(idx[0, :, 1], np.arange(400) % 200 + 200)
        assert (dists[0, :, :2] == 0).all() and not ref["marginal"].any()
    if name.startswith("self"):                               # a query that is itself in p2 finds itself
        assert np.array_equal(idx[0, :, 0], np.arange(idx.shape[1])) and (dists[0, :, 0] == 0).all()
    if name == "pad_P2_3_K4":
        assert (idx[..., 3] == 0).all() and (dists[..., 3] == 0).all() and (dists[..., 2] > 0).all()
    if name == "outside_257x1000":
        lo, hi = c["p2"][0].min(0), c["p2"][0].max(0)
        out = ((c["p1"][0] < lo) | (c["p1"][0] > hi)).any(1)
        assert 80 <= out.sum() <= 90 and float(((c["p1"][0] - hi) / (hi - lo)).max()) > 1.5       # a third outside, by up to two box sizes
    if name == "flat1500":
        from d3ga_amd.knn import _grid
        assert _grid(torch.from_numpy(c["p2"][0].copy()))[3][2] == 1                             # one cell deep
    assert worst <= 1.0, f"{name}: dists off by {worst:.3f} x the bar 4 * 2^-24 d + 2^-149"


def test_queries_that_are_not_finite_end_the_walk_and_insert_nothing_they_cannot_compare():
    """A NaN coordinate makes every distance NaN: nothing is inserted, the row is padding, and the ring walk still ends (it is
    bounded by the grid).  An infinite query is infinitely far from everything: distances inf, in index order."""
    p2 = kr.case("self300_K4")["p2"]
    q = p2[:, :4].copy()
    q[0, 1, 0], q[0, 2, 2], q[0, 3, 1] = np.nan, np.inf, -np.inf
    for method in ("exhaustive", "grid"):
        dists, idx = kr.host_knn_arrays(q, p2, 4, method)
        assert idx[0, 0, 0] == 0 and dists[0, 0, 0] == 0
        assert (dists[0, 1] == 0).all() and (idx[0, 1] == 0).all()
        assert np.isinf(dists[0, 2:]).all() and (idx[0, 2:] == np.arange(4)).all(), method


def test_interp_host_evaluation_is_the_stated_expression():
    rng = np.random.default_rng(5)
    F, D = 11, 6
    p2f = rng.integers(-1, F + 1, (2, 5, 7, 1))               # background, and one index past the end
    bary = rng.uniform(0, 1, p2f.shape + (3,)).astype(np.float32)
    attrs = rng.standard_normal((F, 3, D)).astype(np.float32)
    got = kr.host_interp(p2f, bary, attrs)
    m = (p2f >= 0) & (p2f < F)
    assert (got[~m] == 0).all()
    a = attrs[p2f[m]]                                          # (M,3,D)
    b = bary[m]
    want = (b[:, 0:1] * a[:, 0] + b[:, 1:2] * a[:, 1]) + b[:, 2:3] * a[:, 2]      # numpy float32: one rounding per operation, in this order
    assert want.dtype == np.float32 and np.array_equal(got[m].view(np.int32), want.view(np.int32))


def test_map_pipeline_on_the_host():
    """The float32 map pipeline on the host against its float64 evaluation at the same fragments: the figures behind
    compat_ref.BARS (8 x), which the GPU test holds the device to."""
    s = cr.scene()
    p2f, bary, vn = cr.host_fragments_and_normals()
    assert (p2f >= 0).mean() > 0.2 and (p2f[1][p2f[1] >= 0] >= 200).all() and (p2f[0] < 200).all()
    faces = s["faces"]
    with cr.compat_path():
        cams = cr.shim_cameras(torch)
        verts = torch.from_numpy(s["verts"].copy())
        view = cams.get_world_to_view_transform().transform_points(verts).numpy()               # float32 on the CPU
    packed_faces = np.concatenate([faces, faces + s["verts"].shape[1]])
    attrs = np.concatenate([s["verts"].reshape(-1, 3)[packed_faces], view.reshape(-1, 3)[packed_faces]], -1)      # (2F,3,6)
    maps = kr.host_interp(p2f[..., None], bary[:, :, :, None, :], attrs)[:, :, :, 0]
    nsum = kr.host_interp(p2f[..., None], np.ones_like(bary)[:, :, :, None, :], vn.reshape(-1, 3)[packed_faces])[:, :, :, 0]
    nrm = nsum / np.maximum(np.linalg.norm(nsum, axis=-1, keepdims=True), np.float32(1e-8))
    want = cr.maps64(s["verts"], faces, s["R"], s["t"], cr.normals64(), p2f, bary)
    dev = cr.deviations(maps[..., 0:3], maps[..., 5], nrm, want)
    print("host map pipeline: " + " ".join(f"{k} {v:.2e}" for k, v in sorted(dev.items())))
    for k, v in dev.items():
        assert v <= cr.MEASURED[k], (k, v)
        assert cr.BARS[k] == 8 * cr.MEASURED[k]


# ---- the ABI and the Python layers' refusals ------------------------------------------------------------------------------------------
def test_new_abi_surface_and_refusals():
    import ctypes
    import re
    from d3ga_amd import _lib
    from d3ga_amd.csrc import build as b
    src = open(os.path.join(ROOT, "include", "d3ga.h")).read()
    for name, nargs in (("d3ga_knn_points", 9), ("d3ga_knn_points_grid", 12), ("d3ga_interp_face_attrs", 8)):
        assert name in _lib.EXPORTS and len(_lib._SIGNATURES[name][0]) == nargs and re.search(r"\bint\s+%s\s*\(" % name, src)
    assert "knn.hip" in b.SOURCES and "knn_math.h" in b.HEADERS and "-ffp-contract=off" in b.EXTRA["knn.hip"]
    assert _lib.ABI_VERSION == 112 and _lib.KNN_MAX_K == 16 == int(re.search(r"#define\s+D3GA_KNN_MAX_K\s+(\d+)", src).group(1))
    assert _lib.INTERP_MAX_D == 64 == int(re.search(r"#define\s+D3GA_INTERP_MAX_D\s+(\d+)", src).group(1))
    L = _lib.lib()
    E_NULL, E_SIZE, E_CONFIG = -1, -2, -3
    buf = (ctypes.c_float * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    # refused before any HIP call: host memory stands in for device memory and is never touched
    assert L.d3ga_knn_points(1, 0, 5, 4, None, None, None, None, None) == 0 and L.d3ga_knn_points(0, 5, 5, 4, None, None, None, None, None) == 0
    for kw in ((-1, 1, 1, 4), (1, -1, 1, 4), (1, 1, -1, 4), (1, 1, 1, 0), (1, 1, 1, 17), (65536, 1, 1, 4)):
        assert L.d3ga_knn_points(*kw, p, p, p, p, None) == E_SIZE, kw
    for missing in range(4):
        args = [p, p, p, p]
        args[missing] = None
        assert L.d3ga_knn_points(1, 2, 2, 4, *args, None) == E_NULL, missing
    oh, dims = (ctypes.c_float * 4)(0, 0, 0, 0.5), (ctypes.c_int32 * 3)(2, 2, 2)
    assert L.d3ga_knn_points_grid(0, 5, 4, None, None, None, None, None, None, None, None, None) == 0
    assert L.d3ga_knn_points_grid(2, 2, 17, p, p, p, p, oh, dims, p, p, None) == E_SIZE
    assert L.d3ga_knn_points_grid(2, 2, 4, p, p, p, p, (ctypes.c_float * 4)(0, 0, 0, 0.0), dims, p, p, None) == E_SIZE
    assert L.d3ga_knn_points_grid(2, 2, 4, p, p, p, p, (ctypes.c_float * 4)(0, 0, 0, float("nan")), dims, p, p, None) == E_SIZE
    assert L.d3ga_knn_points_grid(2, 2, 4, p, p, p, p, oh, (ctypes.c_int32 * 3)(2, 0, 2), p, p, None) == E_SIZE
    assert L.d3ga_knn_points_grid(2, 2, 4, p, p, p, p, oh, (ctypes.c_int32 * 3)(2048, 2048, 2048), p, p, None) == E_SIZE
    assert L.d3ga_knn_points_grid(2, 2, 4, p, p, None, p, oh, dims, p, p, None) == E_NULL
    assert L.d3ga_knn_points_grid(2, 2, 4, p, p, p, p, None, dims, p, p, None) == E_NULL
    f = L.d3ga_interp_face_attrs
    assert f(0, 3, 3, None, None, None, None, None) == 0
    for kw in ((-1, 3, 3), (4, -1, 3), (4, 3, 0), (4, 3, 65)):
        assert f(*kw, p, p, p, p, None) == E_SIZE, kw
    assert f(4, 3, 3, None, p, p, p, None) == E_NULL and f(4, 3, 3, p, p, None, p, None) == E_NULL and f(4, 3, 3, p, p, p, None, None) == E_NULL
    assert f(4, 3, 3, ctypes.c_void_p(p.value + 4), p, p, p, None) == E_CONFIG and f(4, 3, 3, p, p, p, ctypes.c_void_p(p.value + 2), None) == E_CONFIG
    assert not any(buf)
    # the Python layers refuse on the host, before they ask for a GPU
    from d3ga_amd import D3GAError, interpolate_face_attributes, knn_points
    pts = torch.zeros(1, 5, 3)
    with pytest.raises(ValueError, match="K = 17"):
        knn_points(pts, pts, K=17)
    for kw, word in ((dict(norm=1), "norm"), (dict(lengths1=torch.tensor([3])), "lengths1"), (dict(lengths2=torch.tensor([2])), "lengths2"),
                     (dict(return_sorted=False), "return_sorted")):
        with pytest.raises(NotImplementedError, match=word):
            knn_points(pts, pts, K=2, **kw)
    with pytest.raises(NotImplementedError, match="D = 2"):
        knn_points(torch.zeros(1, 5, 2), torch.zeros(1, 5, 2))
    with pytest.raises(ValueError):
        knn_points(pts, pts, K=2, method="fast")
    with pytest.raises(D3GAError, match="GPU only"):
        knn_points(pts, pts, K=2, lengths1=torch.tensor([5]))                                   # full lengths are accepted; CPU tensors are not
    with pytest.raises(ValueError):
        interpolate_face_attributes(torch.zeros(1, 2, 2, 1, dtype=torch.int32), torch.zeros(1, 2, 2, 1, 3), torch.zeros(4, 3, 3))
    with pytest.raises(ValueError, match="D = 65"):
        interpolate_face_attributes(torch.zeros(1, 2, 2, 1, dtype=torch.int64), torch.zeros(1, 2, 2, 1, 3), torch.zeros(4, 3, 65))
    with pytest.raises(D3GAError, match="GPU only"):
        interpolate_face_attributes(torch.zeros(1, 2, 2, 1, dtype=torch.int64), torch.zeros(1, 2, 2, 1, 3), torch.zeros(4, 3, 3))
