"""The triangle-mesh rasterizer without a GPU.  pytorch3d cannot be run next to this library, so no golden exists: the float64
oracle (tests/mesh_ref.py, written from DESIGN.md 4.4f) is checked from first principles instead (rays, partition of unity,
rigid motions, a hand-computed triangle), and the g++ build of csrc/mesh_raster_math.h -- the text the kernels run, at
-ffp-contract=off as the device build -- is held to the oracle: pix_to_face exactly away from the marginal pixels, the values
within an eighth of the bars of the GPU tests (mesh_ref.BARS, which are 8 x what this module measures).  Then the marginal
cap, the vertex -> face lists, to_cameras, the ABI surface, its refusals and the Python layer's ValueErrors."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import mesh_ref as mr
from conftest import ROOT, ptr

E_NULL, E_SIZE, E_CONFIG = -1, -2, -3            # D3GA_E_* (include/d3ga.h)
NEW_EXPORTS = ("d3ga_mesh_raster_scratch_bytes", "d3ga_mesh_rasterize", "d3ga_mesh_shade_flat", "d3ga_mesh_vertex_normals", "d3ga_mesh_maps")


@pytest.fixture(scope="module")
def meshcheck():
    src = os.path.join(ROOT, "tests", "hostcheck", "meshcheck.cpp")
    out_dir = os.path.join(ROOT, "tests", "hostcheck", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libmeshcheck.so")
    deps = [src, os.path.join(ROOT, "d3ga_amd", "csrc", "mesh_raster_math.h"), os.path.join(ROOT, "include", "d3ga.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", so])
    lib = ctypes.CDLL(so)
    lib.hc_mesh_rasterize.restype = ctypes.c_int64
    lib.hc_mesh_covered_pairs_plain.restype = ctypes.c_int64
    return lib


def host_run(lib, ref, white=True):
    """Every output of the host build for a case -> dict of arrays (the layout of the entry points)."""
    from d3ga_amd.mesh_render import vertex_face_csr
    c = ref.case
    B, V, F, H, W = ref.B, ref.V, ref.F, ref.H, ref.W
    verts, faces, cams = (np.ascontiguousarray(c[k]) for k in ("verts", "faces", "cams"))
    o = dict(pix=np.full((B, H, W), -7, np.int32), zbuf=np.full((B, H, W), np.nan, np.float32), bary=np.full((B, H, W, 3), np.nan, np.float32))
    o["fragments"] = lib.hc_mesh_rasterize(B, V, F, H, W, ptr(verts), ptr(faces), ptr(cams), ptr(o["pix"]), ptr(o["zbuf"]), ptr(o["bary"]))
    assert o["fragments"] == lib.hc_mesh_covered_pairs_plain(B, V, F, H, W, ptr(verts), ptr(faces), ptr(cams))     # the cell rejection lost nothing
    bg = np.full(3, 1.0 if white else 0.0, np.float32)
    for name, rgb in (("image", None), ("image_rgb", ref.rgb)):
        o[name] = np.full((B, H, W, 3), np.nan, np.float32)
        lib.hc_mesh_shade_flat(B, V, F, H, W, ptr(verts), ptr(faces), ptr(rgb), ptr(cams), ptr(o["pix"]), ptr(o["bary"]), ptr(bg), ptr(o[name]))
    off, idx = vertex_face_csr(faces, V)
    idx = np.ascontiguousarray(np.concatenate([idx, np.zeros(1, np.int32)]))
    o["vn"] = np.full((B, V, 3), np.nan, np.float32)
    lib.hc_mesh_vertex_normals(B, V, F, ptr(verts), ptr(faces), ptr(off), ptr(idx), ptr(o["vn"]))
    for k, ch in (("position", 3), ("normal", 3), ("depth", 1), ("mask", 1)):
        o[k] = np.full((B, H, W, ch), np.nan, np.float32)
    lib.hc_mesh_maps(B, V, F, H, W, ptr(verts), ptr(faces), ptr(o["vn"]), ptr(cams), ptr(o["pix"]), ptr(o["bary"]), ptr(o["position"]),
                     ptr(o["normal"]), ptr(o["depth"]), ptr(o["mask"]))
    return o


def deviations(ref, o, white=True):
    """The largest deviation of every quantity from the oracle on non-marginal pixels (asserts the exact parts)."""
    dev = ref.check_fragments(o["pix"], o["zbuf"], o["bary"])
    dev["image"] = max(ref.check_image(o["image"], white, False), ref.check_image(o["image_rgb"], white, True))
    dev.update(ref.check_maps(o["position"], o["normal"], o["depth"], o["mask"]))
    dev["vertex_normal"] = ref.check_vertex_normals(o["vn"])
    return dev


# ---- the oracle from first principles ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("tri_face1", "interpenetrating", "sphere64", "sphere288_closeup", "batch3"))
def test_oracle_positions_lie_on_the_pixel_rays_and_barycentrics_sum_to_one(name):
    ref = mr.reference(name)
    c = ref.case
    for b, fr in enumerate(ref.frag):
        cam = c["cams"][b].astype(np.float64)
        R, t, (fx, fy, cx, cy) = cam[:9].reshape(3, 3), cam[9:12], cam[12:]
        pos, _, depth, _ = mr.maps_ref(c["verts"][b], c["faces"], c["cams"][b], fr["pix_to_face"], fr["bary"])
        m = fr["covered"]
        assert m.any()
        jj, ii = np.nonzero(m)
        ray = np.stack([(ii + 0.5 - cx) / fx, (jj + 0.5 - cy) / fy, np.ones(len(ii))], -1)      # K^-1 [u, v, 1]
        view = pos[m] @ R.T + t
        assert float(np.abs(view - ray * depth[m]).max()) <= 1e-9
        assert float(np.abs(depth[m][:, 0] - fr["zbuf"][m]).max()) <= 1e-9                      # sum b' z = 1 / sum b / z
        assert float(np.abs(fr["bary"][m].sum(-1) - 1).max()) <= 1e-12
        assert (fr["bary"][m] >= 0).all() and (fr["bary"][~m] == -1).all() and (fr["zbuf"][~m] == -1).all()


@pytest.mark.parametrize("name", ("interpenetrating", "sphere64", "sphere288"))
def test_oracle_is_invariant_under_a_rigid_motion_of_mesh_and_camera(name):
    ref = mr.reference(name)
    c = ref.case
    rng = np.random.default_rng(5)
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    Q *= np.sign(np.linalg.det(Q))
    s = rng.standard_normal(3)
    cam = c["cams"][0].astype(np.float64)
    R, t = cam[:9].reshape(3, 3), cam[9:12]
    moved = c["verts"][0].astype(np.float64) @ Q.T + s                                          # x' = Q x + s
    cam2 = np.concatenate([(R @ Q.T).reshape(9), t - R @ Q.T @ s, cam[12:]])                    # R' x' + t' = R x + t
    got = mr.rasterize_ref(moved, c["faces"], cam2, ref.H, ref.W)
    fr = ref.frag[0]
    m = ~(fr["marginal"] | got["marginal"])
    assert np.array_equal(got["pix_to_face"][m], fr["pix_to_face"][m]) and m.mean() > 0.9
    assert float(np.abs(got["zbuf"][m] - fr["zbuf"][m]).max()) <= 1e-9


def test_fronto_parallel_triangle_by_hand(meshcheck):
    """A right triangle at z = 2 straight in front of the camera, f = 8, principal point (4, 4) in an 8 x 8 frame: screen
    corners (2,2), (6,2), (2,6).  Pixel centres (i + .5, j + .5) with i, j >= 2 and (i + .5) + (j + .5) <= 8, i.e. i + j <= 7:
    rows j = 2, 3, 4, 5 hold 4, 3, 2, 1 pixels -- the pixels with i + j = 7 sit exactly on the hypotenuse (b = 0: inside) -- 10 in
    all.  Depth 2 everywhere.  The normal is cross(x1 - x0, x2 - x0) = (0, 0, +1) for the order below, pointing away from the
    camera at the origin: n.l < 0, colour 0.45; with the other winding n = (0, 0, -1) and at the pixel whose centre is the
    principal point -- none is, so the camera is moved over pixel (3, 3) with cx = cy = 3.5 -- n.l = 1 exactly:
    0.45 + 0.35 + 0.05 = 0.85."""
    H = W = 8
    verts = np.array([[[-0.5, -0.5, 2.0], [0.5, -0.5, 2.0], [-0.5, 0.5, 2.0]]], np.float32)
    cam = mr.cam_row(np.eye(3), np.zeros(3), 8.0, 8.0, 4.0, 4.0)
    for faces, colour in (([[0, 1, 2]], 0.45), ([[0, 2, 1]], None)):
        faces = np.array(faces, np.int32)
        fr = mr.rasterize_ref(verts[0], faces, cam, H, W)
        want = np.zeros((H, W), bool)
        for j in range(2, 6):
            want[j, 2:2 + 6 - j] = True
        assert np.array_equal(fr["covered"], want) and int(fr["covered"].sum()) == 10
        assert float(np.abs(fr["zbuf"][want] - 2.0).max()) <= 1e-12
        assert int(fr["marginal"].sum()) >= 4                                                   # the hypotenuse pixels are flagged
        img = mr.shade_ref(verts[0], faces, cam, fr["pix_to_face"], fr["bary"])
        if colour is not None:
            assert float(np.abs(img[want] - colour).max()) <= 1e-12 and (img[~want] == 1).all()
        else:
            assert float(img[want].min()) > 0.45 + 0.3
    first_verts, first_cam = verts, cam
    # n.l = 1: the camera over the centre of pixel (3, 3), the winding that faces it
    cam = mr.cam_row(np.eye(3), np.zeros(3), 8.0, 8.0, 3.5, 3.5)
    verts = np.array([[[-0.4, -0.4, 2.0], [0.9, -0.4, 2.0], [-0.4, 0.9, 2.0]]], np.float32)
    faces = np.array([[0, 2, 1]], np.int32)
    fr = mr.rasterize_ref(verts[0], faces, cam, H, W)
    assert fr["pix_to_face"][3, 3] == 0 and not fr["marginal"][3, 3]
    pos = mr.maps_ref(verts[0], faces, cam, fr["pix_to_face"], fr["bary"])[0]
    assert float(np.abs(pos[3, 3] - [0, 0, 2]).max()) <= 1e-12
    img = mr.shade_ref(verts[0], faces, cam, fr["pix_to_face"], fr["bary"])
    assert float(np.abs(img[3, 3] - 0.85).max()) <= 1e-12
    off = img[3, 4]                                                                             # one pixel to the right: p = (0.25, 0, 2)
    cos = 2 / np.sqrt(0.25 ** 2 + 4)
    assert float(np.abs(off - (0.45 + 0.35 * cos + 0.05 * (2 * cos * cos - 1) ** 64)).max()) <= 1e-12
    assert float(np.abs(mr.shade_ref(verts[0], faces, cam, fr["pix_to_face"], fr["bary"], white=False)[0, 0]).max()) == 0
    # and the host build: the same pixel in float32, and the 10 pixels of the first triangle (its numbers are exact in float32 too)
    bg = np.ones(3, np.float32)
    for v32, c32, count in ((np.ascontiguousarray(verts), np.ascontiguousarray(cam[None]), None),
                            (np.ascontiguousarray(first_verts), np.ascontiguousarray(first_cam[None]), 10)):
        o = dict(pix=np.empty((1, H, W), np.int32), zbuf=np.empty((1, H, W), np.float32), bary=np.empty((1, H, W, 3), np.float32))
        n = meshcheck.hc_mesh_rasterize(1, 3, 1, H, W, ptr(v32), ptr(faces), ptr(c32), ptr(o["pix"]), ptr(o["zbuf"]), ptr(o["bary"]))
        image = np.empty((1, H, W, 3), np.float32)
        meshcheck.hc_mesh_shade_flat(1, 3, 1, H, W, ptr(v32), ptr(faces), None, ptr(c32), ptr(o["pix"]), ptr(o["bary"]), ptr(bg), ptr(image))
        if count is None:
            assert float(np.abs(image[0, 3, 3] - 0.85).max()) <= 2e-7 and abs(float(o["zbuf"][0, 3, 3]) - 2) <= 2e-7
        else:
            assert n == count and np.array_equal(o["pix"][0] == 0, want) and (o["zbuf"][0][want] == 2).all()


# ---- the host build against the oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mr.CASES)
def test_marginal_pixels_stay_under_the_cap(name):
    share, covered = mr.reference(name).marginal_share()
    print(f"{name}: {share * 100:.2f} % of {covered} covered pixels are marginal")
    assert covered > 0 and share <= mr.MARGINAL_CAP


@pytest.mark.parametrize("name", mr.CASES + ("all_dropped",))
def test_host_build_equals_the_oracle(meshcheck, name):
    ref = mr.reference(name)
    for white in (True, False):
        o = host_run(meshcheck, ref, white)
        dev = deviations(ref, o, white)
    print(f"{name}: fragments {o['fragments']} (oracle {sum(f['fragments'] for f in ref.frag)}) " + " ".join(f"{k} {v:.2e}" for k, v in sorted(dev.items())))
    for k, v in dev.items():
        assert 8 * v <= mr.BARS[k], (k, v)
    if name == "all_dropped":
        assert (o["pix"] == -1).all() and (o["image"] == 0).all() and (o["position"] == 0).all() and (o["mask"] == 0).all()
    if name == "tri_face1":                                   # the mask quirk: face 0 is drawn, and masked out
        assert (o["pix"] == 0).any() and (o["mask"][o["pix"] == 0] == 0).all() and (o["mask"][o["pix"] == 1] == 1).all()
        assert (np.abs(o["position"][o["pix"] == 0]).sum(-1) > 0).all()


def test_dropped_faces_change_nothing(meshcheck):
    base, plus = mr.reference("sphere64"), mr.reference("sphere64_plus_dropped")
    assert plus.F == base.F + 2
    a, b = host_run(meshcheck, base), host_run(meshcheck, plus)
    for k in ("pix", "zbuf", "bary", "image", "position", "depth"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(plus.frag[0]["pix_to_face"], base.frag[0]["pix_to_face"])


# ---- host-side pieces of the Python layer ---------------------------------------------------------------------------------------
def test_vertex_face_lists():
    from d3ga_amd.mesh_render import MeshTopology, vertex_face_csr
    faces = np.array([[0, 1, 2], [2, 1, 4], [4, 4, 0], [2, 0, 1]], np.int32)          # vertex 3 has no face, vertex 5 neither
    off, idx = vertex_face_csr(faces, 6)
    assert off.dtype == np.int32 and idx.dtype == np.int32 and off.tolist() == [0, 3, 6, 9, 9, 12, 12]
    lists = [idx[off[v]:off[v + 1]].tolist() for v in range(6)]
    assert lists == [[0, 2, 3], [0, 1, 3], [0, 1, 3], [], [1, 2, 2], []]
    with pytest.raises(ValueError):
        vertex_face_csr(faces, 4)
    fan = np.array([[0, k, k + 1] for k in range(1, 300)], np.int32)                  # a vertex with many faces
    off, idx = vertex_face_csr(fan, 301)
    assert off[1] == 299 and idx[:299].tolist() == list(range(299)) and idx[off[2]:off[3]].tolist() == [0, 1]
    off, idx = vertex_face_csr(np.zeros((0, 3), np.int32), 3)
    assert off.tolist() == [0, 0, 0, 0] and len(idx) == 0
    for v, f in (mr.sphere(8, 4, 1), mr.sphere(12, 12, 2)):
        off, idx = vertex_face_csr(f, len(v))
        for k in range(len(v)):
            assert idx[off[k]:off[k + 1]].tolist() == sorted(np.flatnonzero((f == k).any(1)).tolist())
    t = MeshTopology(torch.from_numpy(fan.astype(np.int64))[None])
    assert t.F == 299 and t.min_verts == 301
    with pytest.raises(ValueError):
        t.csr(300, "cpu")
    off2, idx2 = t.csr(305, "cpu")
    assert off2.dtype == torch.int32 and off2.shape == (306,) and off2[-1] == 3 * 299 and idx2.shape == (3 * 299,)


def test_to_cameras_agrees_with_numpy():
    from d3ga_amd import MeshCameras, to_cameras
    rng = np.random.default_rng(2)
    frames = []
    for k in range(3):
        R, t = mr.look_at(rng.standard_normal(3) * 2 + [0, 0, 4])
        w2c = np.eye(4)
        w2c[:3, :3], w2c[:3, 3] = R, t
        K = np.array([[900.0 + k, 0.3, 310.5], [0, 905.0, 255.25 + k], [0, 0, 1]])
        frames.append({"K": torch.from_numpy(K).float(), "c2w": np.linalg.inv(w2c).tolist(), "crop": torch.tensor([5, 7, 640, 480])})
    cams = to_cameras(frames, device="cpu")
    assert (cams.H, cams.W, cams.B, len(cams)) == (480, 640, 3, 3) and cams.data.dtype == torch.float32 and cams.data.shape == (3, 16)
    for k, f in enumerate(frames):
        w2c = np.linalg.inv(np.array(f["c2w"], np.float64))
        K = f["K"].double().numpy()
        want = np.concatenate([w2c[:3, :3].reshape(9), w2c[:3, 3], [K[0, 0], K[1, 1], K[0, 2], K[1, 2]]]).astype(np.float32)
        assert np.array_equal(cams.data[k].numpy(), want)
        one = to_cameras(f, device="cpu")
        assert one.B == 1 and torch.equal(one.data[0], cams.data[k])
    raw = MeshCameras(torch.eye(3), [0.0, 0.0, 1.0], np.diag([2.0, 3.0, 1.0]), (4, 5), device="cpu")
    assert raw.data.tolist() == [[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 1, 2, 3, 0, 0]] and (raw.H, raw.W) == (4, 5)
    bad = [lambda: to_cameras([], device="cpu"), lambda: to_cameras({"K": np.eye(3), "c2w": np.eye(4)}, device="cpu"),
           lambda: to_cameras([frames[0], {**frames[1], "crop": [0, 0, 64, 48]}], device="cpu"),
           lambda: to_cameras({**frames[0], "c2w": np.eye(3)}, device="cpu"),
           lambda: MeshCameras(np.eye(3), np.zeros(3), np.eye(3), (0, 5), device="cpu"),
           lambda: MeshCameras(np.eye(3), np.zeros(3), np.eye(3), (5, 16385), device="cpu"),
           lambda: MeshCameras(np.zeros((2, 3, 3)), np.zeros((3, 3)), np.eye(3), (5, 5), device="cpu"),
           lambda: MeshCameras(np.eye(3), np.full(3, np.nan), np.eye(3), (5, 5), device="cpu"),
           lambda: MeshCameras(np.eye(3), np.zeros(3), np.eye(3), 5, device="cpu")]
    for i, fn in enumerate(bad):
        with pytest.raises(ValueError):
            fn()
            pytest.fail(f"case {i} was accepted")


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
def test_new_abi_surface():
    from d3ga_amd import _lib
    src = open(os.path.join(ROOT, "include", "d3ga.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], capture_output=True, text=True, check=True).stdout
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert hasattr(_lib.lib(), name)
        assert re.search(r"\bT %s$" % name, out, flags=re.M), name
    assert sorted(n for n in _lib.EXPORTS if n.startswith("d3ga_mesh_")) == sorted(NEW_EXPORTS)           # exactly the five
    assert sorted(set(re.findall(r"\b(d3ga_mesh_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))) == sorted(NEW_EXPORTS)
    assert _lib.ABI_VERSION == 112 and re.search(r"#define\s+D3GA_VERSION\s+112\b", src) and _lib.lib().d3ga_version() == 112
    assert _lib.MESH_MAX_SIDE == 16384 == int(re.search(r"#define\s+D3GA_MESH_MAX_SIDE\s+(\d+)", src).group(1))
    assert _lib.MESH_CAM_FLOATS == 16 == int(re.search(r"#define\s+D3GA_MESH_CAM_FLOATS\s+(\d+)", src).group(1))
    build = open(os.path.join(ROOT, "d3ga_amd", "csrc", "build.py")).read()
    assert "mesh_raster.hip" in build and "mesh_raster_math.h" in build and "-fhip-fp32-correctly-rounded-divide-sqrt" in build
    n = [len(_lib._SIGNATURES[k][0]) for k in NEW_EXPORTS]
    assert n == [6, 13, 14, 9, 16]
    import d3ga_amd
    for name in ("Renderer", "to_cameras", "MeshCameras", "MeshTopology", "MeshScratch", "rasterize_meshes", "Fragments", "vertex_normals"):
        assert hasattr(d3ga_amd, name) and name in d3ga_amd.__all__


def test_scratch_bytes():
    from d3ga_amd import _lib
    f = _lib.lib().d3ga_mesh_raster_scratch_bytes
    n = ctypes.c_size_t()
    assert f(1, 3, 1, 8, 8, ctypes.byref(n)) == 0 and n.value >= 8 * 64 + 48 + 4 * 256 + 4 + 16
    assert f(6, 7502, 15000, 1080, 1920, ctypes.byref(n)) == 0
    assert n.value >= 6 * 1080 * 1920 * 8 + 6 * 15000 * 52 and n.value <= 6 * 1080 * 1920 * 8 + 6 * 15000 * 64 + 8192
    assert f(0, 0, 0, 1, 1, ctypes.byref(n)) == 0 and n.value >= 16
    assert f(1, 1, 1, 16384, 16384, ctypes.byref(n)) == 0 and n.value >= 2 ** 31                           # no 32-bit overflow
    assert f(1, 3, 1, 8, 8, None) == E_NULL
    for kw in ((-1, 3, 1, 8, 8), (1, -3, 1, 8, 8), (1, 3, -1, 8, 8), (1, 3, 1, 0, 8), (1, 3, 1, 8, 0), (1, 3, 1, 16385, 8), (1, 3, 1, 8, 16385),
               (2, 3, 2 ** 30, 8, 8), (2 ** 16, 3, 2 ** 15, 8, 8)):
        assert f(*kw, ctypes.byref(n)) == E_SIZE, kw
    assert f(1, 3, 2 ** 31 - 1, 8, 8, ctypes.byref(n)) == 0


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """The refusals happen before any HIP call: host buffers stand in for device memory and are never touched."""
    from d3ga_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    odd = ctypes.c_void_p(p.value + 2)
    bg = (ctypes.c_float * 3)(1, 1, 1)
    sizes = dict(B=1, V=3, F=1, H=2, W=2)
    bad_sizes = [dict(B=-1), dict(V=-1), dict(F=-1), dict(H=0), dict(W=0), dict(H=-4), dict(H=16385), dict(W=16385), dict(B=2, F=2 ** 30)]
    calls = {
        "rasterize": (L.d3ga_mesh_rasterize, dict(**sizes, verts=p, faces=p, cams=p, scratch=p, pix_to_face=p, zbuf=p, bary=p),
                      ("verts", "faces", "cams", "scratch", "pix_to_face"), ("zbuf", "bary")),
        "shade": (L.d3ga_mesh_shade_flat, dict(**sizes, verts=p, faces=p, verts_rgb=p, cams=p, pix_to_face=p, bary=p, bg=bg, image=p),
                  ("verts", "faces", "cams", "pix_to_face", "bary", "bg", "image"), ("verts_rgb",)),
        "maps": (L.d3ga_mesh_maps, dict(**sizes, verts=p, faces=p, vertex_normals=p, cams=p, pix_to_face=p, bary=p, position=p, normal=p,
                                        depth=p, mask=p),
                 ("verts", "faces", "vertex_normals", "cams", "pix_to_face", "bary"), ("position", "normal", "depth", "mask")),
    }
    for what, (fn, ok, required, optional) in calls.items():
        call = lambda **kw: fn(*{**ok, **kw}.values(), None)
        for kw in bad_sizes:
            assert call(**kw) == E_SIZE, (what, kw)
        for name in required:
            assert call(**{name: None}) == E_NULL, (what, name)
        for name in required + optional:
            if name != "bg":
                assert call(**{name: odd}) == E_CONFIG, (what, name)
    call = lambda **kw: L.d3ga_mesh_rasterize(*{**calls["rasterize"][1], **kw}.values(), None)
    assert call(scratch=ctypes.c_void_p(p.value + 8)) == E_CONFIG                                # 16-byte alignment
    assert call(B=0) == 0 and call(B=0, verts=None, faces=None, V=0, F=0) == 0                   # nothing to do, nothing launched
    call = lambda **kw: L.d3ga_mesh_maps(*{**calls["maps"][1], **kw}.values(), None)
    assert call(position=None, normal=None, depth=None, mask=None) == E_NULL
    ok = dict(B=1, V=3, F=1, verts=p, faces=p, csr_offsets=p, csr_faces=p, normals=p)
    call = lambda **kw: L.d3ga_mesh_vertex_normals(*{**ok, **kw}.values(), None)
    for kw in (dict(B=-1), dict(V=-1), dict(F=-1), dict(B=2, F=2 ** 30)):
        assert call(**kw) == E_SIZE, kw
    for name in ("verts", "faces", "csr_offsets", "csr_faces", "normals"):
        assert call(**{name: None}) == E_NULL and call(**{name: odd}) == E_CONFIG, name
    assert call(B=0) == 0 and call(V=0, verts=None, csr_offsets=None, normals=None) == 0
    assert not any(buf)


def test_python_layer_validates_on_the_host():
    from d3ga_amd import D3GAError, MeshCameras, MeshScratch, MeshTopology, Renderer, rasterize_meshes, vertex_normals
    cams = MeshCameras(np.eye(3), np.zeros(3), np.diag([8.0, 8.0, 1.0]), (6, 8), device="cpu")
    two = MeshCameras(np.eye(3), np.zeros((2, 3)), np.eye(3), (6, 8), device="cpu")
    verts, faces = torch.zeros(1, 4, 3), torch.tensor([[0, 1, 2], [1, 2, 3]])
    r = Renderer()
    sized = Renderer(white_background=False)
    sized.resize(6, 9)
    bad = [
        lambda: r.render(None, verts, faces),                                                   # cameras
        lambda: r.render(two, verts, faces),
        lambda: r.render(cams, verts[0], faces),                                                # vertices
        lambda: r.render(cams, verts.double(), faces),
        lambda: r.render(cams, verts.numpy(), faces),
        lambda: r.render(cams, torch.zeros(1, 4, 2), faces),
        lambda: r.render(cams, torch.zeros(1, 3, 3), faces),                                    # faces name vertex 3
        lambda: r.render(cams, verts, faces.float()),                                           # faces
        lambda: r.render(cams, verts, faces.int().reshape(2, 3, 1)),
        lambda: r.render(cams, verts, torch.tensor([[0, 1, -2]])),
        lambda: r.render(cams, verts, faces[None].expand(2, 2, 3)),
        lambda: r.render(cams, verts, [[0, 1, 2]]),
        lambda: r.maps(cams, verts, None),
        lambda: rasterize_meshes(cams, verts, faces.short()),
        lambda: sized(cams, verts, faces),                                                      # resize disagrees with the cameras
        lambda: sized.map(cams, verts, faces),
        lambda: sized.resize(0, 4),
        lambda: r.resize(4, 16385),
        lambda: vertex_normals(verts[0], faces),
        lambda: vertex_normals(torch.zeros(1, 3, 3), faces),
        lambda: MeshTopology(np.zeros((2, 4), np.int32)),
        lambda: MeshTopology(np.zeros((2, 2, 3), np.int32)),
    ]
    for i, fn in enumerate(bad):
        with pytest.raises(ValueError):
            fn()
            pytest.fail(f"case {i} was accepted")
    # everything fits, but the tensors live on the CPU: require_cuda's refusal, a ValueError and a D3GAError at once
    for fn in (lambda: r(cams, verts, faces), lambda: r.map(cams, verts, faces[None]), lambda: r.render(cams, verts, faces.int()),
               lambda: rasterize_meshes(cams, verts, MeshTopology(faces)), lambda: vertex_normals(verts, faces)):
        with pytest.raises(ValueError) as info:
            fn()
        assert isinstance(info.value, D3GAError) and "GPU only" in str(info.value)
    assert Renderer().white_background is True and list(sized._bg) == [0.0, 0.0, 0.0] and list(r._bg) == [1.0, 1.0, 1.0]
    assert r.topology(faces) is r.topology(faces)                                               # cached on the tensor
    other = faces.clone()
    assert r.topology(other) is not r.topology(faces)
