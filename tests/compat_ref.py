"""What the tests of compat/pytorch3d share: the scene (two closed 200-face meshes, two cameras, 70 x 90; a 3000-point cloud), the
map pipeline of the reference's recorder/mesh_renderer.py:69-100 in float64, and the same pipeline in float32 on the host
(fragments and vertex normals from the g++ build of csrc/mesh_raster_math.h, the shim's transform on CPU tensors, the g++
evaluation of d3ga_interp_face_attrs): its deviation from the float64 evaluation, times 8, is the bar of the GPU test."""
import ctypes
import os
import subprocess
import sys

import numpy as np

import mesh_ref as mr
from conftest import ROOT

COMPAT = os.path.join(ROOT, "compat")
H, W = 70, 90
# The largest deviations of the float32 host pipeline from the float64 evaluation at the same fragments and float32 inputs
# (tests/test_pytorch3d_compat_host.py::test_map_pipeline_on_the_host prints them and holds the host build to these); the GPU
# test's bars are 8 x these, the project's rule (tests/test_gpu_point_render.py).
MEASURED = {"position": 9.9e-8, "depth": 3.1e-7, "normal": 8.6e-8}
BARS = {k: 8 * v for k, v in MEASURED.items()}
# the two tinycudann configurations that are built: the encoding alone, and as models/mlp.py:166-179 writes it
SH4 = {"otype": "SphericalHarmonics", "degree": 4}
COMPOSITE = {"otype": "Composite", "nested": [{"n_dims_to_encode": 3, "otype": "SphericalHarmonics", "degree": 4}, {"otype": "Identity"}]}


class compat_path:
    """`with compat_path():` puts compat/ first on sys.path and drops the shadowed packages from sys.modules on both sides."""
    NAMES = ("pytorch3d", "tinycudann")

    def _forget(self):
        for name in [m for m in sys.modules if m.split(".")[0] in self.NAMES]:
            del sys.modules[name]

    def __enter__(self):
        self._forget()
        sys.path.insert(0, COMPAT)
        return self

    def __exit__(self, *exc):
        sys.path.remove(COMPAT)
        self._forget()


def closed_sphere(nu=10, nv=11, seed=5, bump=0.05):
    """A closed bumpy sphere: two poles and nv - 1 rings of nu vertices, 2 nu (nv - 1) = 200 faces, outward winding."""
    rng = np.random.default_rng(seed)
    theta = np.linspace(0, np.pi, nv + 1)[1:-1, None]
    phi = (np.arange(nu) * (2 * np.pi / nu))[None, :]
    r = 1 + bump * np.cos(2 * theta + rng.uniform(0, 6)) * np.cos(3 * phi + rng.uniform(0, 6)) + 0.01 * rng.uniform(-1, 1, (nv - 1, nu))
    ring = np.stack([r * np.sin(theta) * np.cos(phi), r * np.cos(theta) * np.ones_like(phi), r * np.sin(theta) * np.sin(phi)], -1).reshape(-1, 3)
    verts = np.concatenate([[[0, 1.0, 0]], ring, [[0, -1.0, 0]]]).astype(np.float32)
    idx = 1 + np.arange((nv - 1) * nu).reshape(nv - 1, nu)
    nxt = np.roll(idx, -1, 1)
    faces = [np.stack([np.zeros(nu, int), nxt[0], idx[0]], -1)]
    a, b, c, d = idx[:-1], nxt[:-1], idx[1:], nxt[1:]
    faces += [np.stack([a, b, c], -1).reshape(-1, 3), np.stack([b, d, c], -1).reshape(-1, 3)]
    last = len(verts) - 1
    faces.append(np.stack([np.full(nu, last), idx[-1], nxt[-1]], -1))
    return verts, np.concatenate(faces).astype(np.int64)


_SCENE = {}


def scene():
    """-> dict(verts (2,V,3) float32, faces (F,3) int64, R (2,3,3), t (2,3), K (2,3,3) float32 OpenCV cameras, cams (2,16) float32 rows of
    the kernels, points (2,3000,3) float32).  Built once, read-only."""
    if not _SCENE:
        v0, f = closed_sphere(seed=5)
        v1, _ = closed_sphere(seed=6, bump=0.08)
        Rs, ts, Ks, rows = [], [], [], []
        for eye, focal in (((0.9, 1.1, -2.2), 62.0), ((-1.6, 0.3, 1.9), 58.0)):
            R, t = mr.look_at(eye)
            K = np.array([[focal, 0, 0.5 * W + 0.3], [0, 1.03 * focal, 0.5 * H - 0.2], [0, 0, 1]])
            Rs.append(R); ts.append(t); Ks.append(K)
            rows.append(mr.cam_row(R, t, K[0, 0], K[1, 1], K[0, 2], K[1, 2]))
        cloud = np.stack([mr.sphere(60, 49, 31)[0][:3000], mr.sphere(60, 49, 32)[0][:3000]])
        s = dict(verts=np.stack([v0, v1]), faces=f, R=np.stack(Rs).astype(np.float32), t=np.stack(ts).astype(np.float32),
                 K=np.stack(Ks).astype(np.float32), cams=np.stack(rows), points=np.ascontiguousarray(cloud, np.float32))
        assert f.shape == (200, 3) and s["points"].shape == (2, 3000, 3)
        for a in s.values():
            a.setflags(write=False)
        _SCENE.update(s)
    return _SCENE


def shim_cameras(torch, device="cpu", n=2):
    """cameras_from_opencv_projection of the scene's first n cameras (call inside compat_path)"""
    from pytorch3d.utils import cameras_from_opencv_projection
    s = scene()
    t = lambda a: torch.from_numpy(a[:n].copy()).to(device)
    return cameras_from_opencv_projection(t(s["R"]), t(s["t"]), t(s["K"]), torch.tensor([[H, W]] * n, dtype=torch.int32, device=device))


def maps64(verts, faces, R, t, normals64, pix_to_face, bary):
    """The map pipeline in float64 at given fragments: verts (N,V,3) float32, pix_to_face (N,H,W) packed int64, bary (N,H,W,3)
    float32, normals64 (N,V,3) float64 -> position (N,H,W,3), view depth (N,H,W), normal (N,H,W,3) (normalized, clamp 1e-8);
    0 at background pixels.  pytorch3d's view space: +x left, +y up, +z forward."""
    N, V = verts.shape[:2]
    F = len(faces)
    v = verts.astype(np.float64)
    view = np.einsum("nij,nvj->nvi", R.astype(np.float64), v) + t.astype(np.float64)[:, None, :]
    view = view * np.array([-1.0, -1.0, 1.0])
    pos, depth, nrm = np.zeros(pix_to_face.shape + (3,)), np.zeros(pix_to_face.shape), np.zeros(pix_to_face.shape + (3,))
    m = pix_to_face >= 0
    n_of, f_of = pix_to_face[m] // F, pix_to_face[m] % F
    corner = faces[f_of]                                        # (M,3) vertex indices
    b = bary.astype(np.float64)[m]
    pos[m] = (b[:, :, None] * v[n_of[:, None], corner]).sum(1)
    depth[m] = (b * view[n_of[:, None], corner][:, :, 2]).sum(1)
    s = normals64[n_of[:, None], corner].sum(1)
    nrm[m] = s / np.maximum(np.linalg.norm(s, axis=1, keepdims=True), 1e-8)
    return pos, depth, nrm


def normals64():
    s = scene()
    return np.stack([mr.vertex_normals_ref(s["verts"][n], s["faces"]) for n in range(2)])


def _meshcheck():
    src = os.path.join(ROOT, "tests", "hostcheck", "meshcheck.cpp")
    out_dir = os.path.join(ROOT, "tests", "hostcheck", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libmeshcheck.so")
    deps = [src, os.path.join(ROOT, "d3ga_amd", "csrc", "mesh_raster_math.h"), os.path.join(ROOT, "include", "d3ga.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", so])
    lib = ctypes.CDLL(so)
    lib.hc_mesh_rasterize.restype = ctypes.c_int64
    return lib


def host_fragments_and_normals():
    """The g++ build of the rasterizer and of the vertex normals on the scene -> (pix_to_face (2,H,W) packed int64, bary (2,H,W,3),
    vertex normals (2,V,3) float32)"""
    from d3ga_amd.mesh_render import vertex_face_csr
    s = scene()
    lib = _meshcheck()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    verts, faces, cams = np.ascontiguousarray(s["verts"]), np.ascontiguousarray(s["faces"], np.int32), np.ascontiguousarray(s["cams"])
    B, V, F = 2, verts.shape[1], len(faces)
    pix, zbuf, bary = np.full((B, H, W), -9, np.int32), np.full((B, H, W), np.nan, np.float32), np.full((B, H, W, 3), np.nan, np.float32)
    lib.hc_mesh_rasterize(B, V, F, H, W, ptr(verts), ptr(faces), ptr(cams), ptr(pix), ptr(zbuf), ptr(bary))
    off, idx = vertex_face_csr(faces, V)
    idx = np.ascontiguousarray(np.concatenate([idx, np.zeros(1, np.int32)]))
    vn = np.full((B, V, 3), np.nan, np.float32)
    lib.hc_mesh_vertex_normals(B, V, F, ptr(verts), ptr(faces), ptr(off), ptr(idx), ptr(vn))
    packed = np.where(pix >= 0, pix.astype(np.int64) + np.arange(B)[:, None, None] * F, -1)
    return packed, bary, vn


def deviations(pos, depth, nrm, want):
    """largest absolute deviations of float32 maps (numpy) from maps64's"""
    return {k: float(np.abs(np.asarray(g, np.float64) - w).max()) for k, g, w in zip(("position", "depth", "normal"), (pos, depth, nrm), want)}
