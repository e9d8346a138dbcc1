"""Triangle-mesh views and maps on the device: the reference's recorder/mesh_renderer.py::Renderer (a pytorch3d MeshRasterizer
+ HardFlatShader, and Renderer.map's position / normal / depth / mask maps) and PCRenderer.to_cameras
(recorder/pc_renderer.py:33-56), without pytorch3d: a forward-only rasterizer in HIP (csrc/mesh_raster.hip).  The semantics are
stated in DESIGN.md 4.4f; they are this library's specification of record (pytorch3d cannot be run next to it).

    cameras = to_cameras(frame)                       # K, c2w, crop of a frame dict, or a list of frames
    renderer = Renderer(white_background=True)
    image = renderer(cameras, vertices, faces)        # (H,W,3), element 0, as the reference returns it
    pos, normal, depth, mask = renderer.map(cameras, vertices, faces)

`vertices` is (B,V,3) with one camera per element and ONE face list for the batch; `render` / `maps` return all B elements.
There is no backward: the reference only ever uses these outputs detached, and inputs that require grad are detached here.
GPU tensors only.  No call synchronises with the host, except the first call with a faces tensor that lives on the device
(its vertex -> face lists are built on the host, once per tensor).  With `out=` and `scratch=` nothing is allocated, so a
captured step can contain `render` and `maps`.

Two quirks of the reference are kept: the normal map is normalize(n_v0 + n_v1 + n_v2) of the winning face,
constant over the face, and the mask is `pix_to_face > 0`, so pixels won by face 0 have mask 0.  One departure: a face with a
vertex at view depth <= 0.01 is dropped, not clipped.
"""
import ctypes
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._lib import D3GAError, check, dptr, require_cuda, stream_handle

Fragments = namedtuple("Fragments", ["pix_to_face", "zbuf", "bary_coords"])


class MeshRenderDeviceError(D3GAError, ValueError):
    """A tensor that is not on the current GPU: a D3GAError as everywhere in this package, and a ValueError as every other
    argument error of this module."""


def _device(what, *tensors):
    try:
        require_cuda(*tensors)
    except D3GAError as e:
        raise MeshRenderDeviceError(f"{what}: {e}") from None


def _host64(what, name, x, shape_tail):
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    a = np.asarray(x, dtype=np.float64)
    if a.shape[-len(shape_tail):] != shape_tail or a.ndim not in (len(shape_tail), len(shape_tail) + 1):
        raise ValueError(f"{what}: expected {name} {shape_tail} or (B,{','.join(map(str, shape_tail))}), got {a.shape}")
    return a.reshape((-1,) + shape_tail)


class MeshCameras:
    """B pinhole cameras with OpenCV axes (+x right, +y down, +z forward) and one image size: x_cam = R x + t,
    u = fx x/z + cx, v = fy y/z + cy; the skew K[0,1] is ignored.  R (3,3) or (B,3,3) world to camera, t (3,) or (B,3),
    K (3,3) or (B,3,3), image_size (H, W).  `data` is the (B,16) float32 device tensor the kernels read."""

    def __init__(self, R, t, K, image_size, device="cuda"):
        what = "MeshCameras"
        R, t, K = _host64(what, "R", R, (3, 3)), _host64(what, "t", t, (3,)), _host64(what, "K", K, (3, 3))
        B = max(len(R), len(t), len(K))
        for name, a in (("R", R), ("t", t), ("K", K)):
            if len(a) not in (1, B):
                raise ValueError(f"{what}: {name} holds {len(a)} cameras, the others {B}")
        try:
            H, W = (int(v) for v in image_size)
        except (TypeError, ValueError):
            raise ValueError(f"{what}: image_size must be (H, W), got {image_size!r}") from None
        if not (1 <= H <= _lib.MESH_MAX_SIDE and 1 <= W <= _lib.MESH_MAX_SIDE):
            raise ValueError(f"{what}: image size {H} x {W} outside 1 .. {_lib.MESH_MAX_SIDE}")
        rows = np.empty((B, _lib.MESH_CAM_FLOATS), np.float64)
        rows[:, 0:9] = np.broadcast_to(R, (B, 3, 3)).reshape(B, 9)
        rows[:, 9:12] = np.broadcast_to(t, (B, 3))
        K = np.broadcast_to(K, (B, 3, 3))
        rows[:, 12], rows[:, 13], rows[:, 14], rows[:, 15] = K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]
        if not np.isfinite(rows).all():
            raise ValueError(f"{what}: R, t and K must be finite")
        self.H, self.W, self.B = H, W, B
        self.data = torch.from_numpy(rows.astype(np.float32)).to(device)

    def __len__(self):
        return self.B


def to_cameras(frame_or_frames, device="cuda"):
    """PCRenderer.to_cameras for one frame dict or a list of them (one image size): reads "K" (the original, un-cropped
    intrinsics), "c2w" and "crop" (H = crop[-1], W = crop[-2]); w2c = inv(c2w) in float64 on the host."""
    what = "to_cameras"
    frames = [frame_or_frames] if isinstance(frame_or_frames, dict) else list(frame_or_frames)
    if not frames:
        raise ValueError(f"{what}: no frame")
    Rs, ts, Ks, size = [], [], [], None
    for f in frames:
        for key in ("K", "c2w", "crop"):
            if key not in f:
                raise ValueError(f"{what}: the frame has no {key!r}")
        c2w = _host64(what, "c2w", f["c2w"], (4, 4))
        if len(c2w) != 1:
            raise ValueError(f"{what}: one c2w per frame, got {c2w.shape}")
        w2c = np.linalg.inv(c2w[0])
        crop = f["crop"].detach().cpu().numpy() if torch.is_tensor(f["crop"]) else np.asarray(f["crop"])
        hw = (int(crop.reshape(-1)[-1]), int(crop.reshape(-1)[-2]))
        if size is not None and hw != size:
            raise ValueError(f"{what}: frames of sizes {size} and {hw} in one batch")
        size = hw
        K = _host64(what, "K", f["K"], (3, 3))
        if len(K) != 1:
            raise ValueError(f"{what}: one K per frame, got {K.shape}")
        Rs.append(w2c[:3, :3]); ts.append(w2c[:3, 3]); Ks.append(K[0])
    return MeshCameras(np.stack(Rs), np.stack(ts), np.stack(Ks), size, device=device)


def vertex_face_csr(faces, n_verts):
    """The faces of every vertex as (offsets (n_verts+1,), face indices) int32 numpy arrays: vertex v's faces are
    indices[offsets[v]:offsets[v+1]], ascending (a face that names v twice appears twice)."""
    faces = np.asarray(faces).reshape(-1, 3)
    corners = faces.reshape(-1).astype(np.int64)
    order = np.argsort(corners, kind="stable")
    counts = np.bincount(corners, minlength=n_verts)
    if len(counts) != n_verts:
        raise ValueError(f"vertex_face_csr: faces name vertex {len(counts) - 1}, there are {n_verts}")
    offsets = np.zeros(n_verts + 1, np.int64)
    np.cumsum(counts, out=offsets[1:])
    if offsets[-1] >= 2 ** 31:
        raise ValueError("vertex_face_csr: too many faces")
    return offsets.astype(np.int32), (order // 3).astype(np.int32)


class MeshTopology:
    """A face list on the device, int32 (F,3), with its vertex -> face lists (built on the host, once: topology is static).
    faces: (F,3) or (1,F,3), int32 or int64, tensor or array."""

    def __init__(self, faces):
        what = "MeshTopology"
        f = faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)
        if f.ndim == 3 and f.shape[0] == 1:
            f = f[0]
        if f.ndim != 2 or f.shape[1] != 3:
            raise ValueError(f"{what}: expected faces (F,3) or (1,F,3), got {tuple(f.shape)}")
        if f.dtype not in (np.int32, np.int64):
            raise ValueError(f"{what}: faces must be int32 or int64, got {f.dtype}")
        if f.size and (f.min() < 0 or f.max() >= 2 ** 31 - 1):
            raise ValueError(f"{what}: face indices must lie in [0, 2^31 - 1)")
        self.F = int(f.shape[0])
        self.min_verts = int(f.max()) + 1 if f.size else 0
        self._host = np.ascontiguousarray(f, dtype=np.int32)
        self._faces, self._csr = {}, {}

    def faces(self, device):
        """The (F,3) int32 faces on `device` (uploaded on first use)."""
        device = torch.device(device)
        if device not in self._faces:
            self._faces[device] = torch.from_numpy(self._host if self.F else np.zeros((1, 3), np.int32)).to(device)[:self.F]
        return self._faces[device]

    def csr(self, V, device):
        """(offsets (V+1,), faces) int32 tensors on `device` for meshes of V vertices."""
        if V < self.min_verts:
            raise ValueError(f"MeshTopology: the faces name vertex {self.min_verts - 1}, the mesh has {V} vertices")
        key = (V, torch.device(device))
        if key not in self._csr:
            off, idx = vertex_face_csr(self._host, V)
            if idx.size == 0:
                idx = np.zeros(1, np.int32)                   # never read: every list is empty
            self._csr[key] = (torch.from_numpy(off).to(device), torch.from_numpy(idx).to(device))
        return self._csr[key]


class MeshScratch:
    """Everything `rasterize_meshes`, `Renderer.render` and `Renderer.maps` need besides their outputs, for one problem size:
    the rasterizer's scratch, the fragments and the vertex normals.  Reusable from call to call (nothing in it needs to be
    clean), which is what a captured step wants."""

    def __init__(self, B, V, F, H, W, device="cuda"):
        n = ctypes.c_size_t()
        check(_lib.lib().d3ga_mesh_raster_scratch_bytes(B, V, F, H, W, ctypes.byref(n)), "d3ga_mesh_raster_scratch_bytes")
        self.key = (B, V, F, H, W)
        self.raw = torch.empty(n.value, dtype=torch.uint8, device=device)
        self.pix_to_face = torch.empty(B, H, W, dtype=torch.int32, device=device)
        self.zbuf = torch.empty(B, H, W, dtype=torch.float32, device=device)
        self.bary = torch.empty(B, H, W, 3, dtype=torch.float32, device=device)
        self.normals = torch.empty(B, V, 3, dtype=torch.float32, device=device)


def _topology(what, faces):
    if isinstance(faces, MeshTopology):
        return faces
    if not torch.is_tensor(faces) and not isinstance(faces, np.ndarray):
        raise ValueError(f"{what}: faces must be a tensor, an array or a MeshTopology, got {type(faces).__name__}")
    return MeshTopology(faces)


def _inputs(what, cameras, vertices, topo, scratch):
    if not isinstance(cameras, MeshCameras):
        raise ValueError(f"{what}: cameras must be MeshCameras (to_cameras), got {type(cameras).__name__}")
    if not torch.is_tensor(vertices):
        raise ValueError(f"{what}: vertices must be a tensor, got {type(vertices).__name__}")
    if vertices.dim() != 3 or vertices.shape[-1] != 3:
        raise ValueError(f"{what}: expected vertices (B,V,3), got {tuple(vertices.shape)}")
    if vertices.dtype != torch.float32:
        raise ValueError(f"{what}: vertices must be float32, got {vertices.dtype}")
    B, V = vertices.shape[0], vertices.shape[1]
    if B != cameras.B:
        raise ValueError(f"{what}: {B} meshes but {cameras.B} cameras")
    if V < topo.min_verts:
        raise ValueError(f"{what}: the faces name vertex {topo.min_verts - 1}, the meshes have {V} vertices")
    if B * topo.F >= 2 ** 31:
        raise ValueError(f"{what}: {B} x {topo.F} faces are more than the 2^31 - 1 accepted")
    _device(what, vertices, cameras.data)
    key = (B, V, topo.F, cameras.H, cameras.W)
    if scratch is None:
        scratch = MeshScratch(*key, device=vertices.device)
    elif not isinstance(scratch, MeshScratch) or scratch.key != key:
        raise ValueError(f"{what}: the scratch is for (B,V,F,H,W) = {getattr(scratch, 'key', None)}, the call is {key}")
    elif scratch.raw.device != vertices.device:
        raise ValueError(f"{what}: the scratch is on {scratch.raw.device}, the vertices on {vertices.device}")
    return vertices.detach().contiguous(), key, scratch


def _out(what, name, out, shape, device):
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if not torch.is_tensor(out) or tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or not out.is_contiguous() or \
            out.device != device:
        raise ValueError(f"{what}: {name} must be a contiguous float32 tensor {tuple(shape)} on {device}")
    return out


def _rasterize(verts, cameras, topo, key, scratch):
    B, V, F, H, W = key
    check(_lib.lib().d3ga_mesh_rasterize(B, V, F, H, W, dptr(verts), dptr(topo.faces(verts.device)), dptr(cameras.data), dptr(scratch.raw),
                                         dptr(scratch.pix_to_face), dptr(scratch.zbuf), dptr(scratch.bary), stream_handle()),
          "d3ga_mesh_rasterize")


def rasterize_meshes(cameras, vertices, faces, scratch=None):
    """-> Fragments(pix_to_face (B,H,W) int32, zbuf (B,H,W), bary_coords (B,H,W,3)): per pixel the index into `faces` of the
    nearest covering face, its depth 1 / sum b_i / z_i and its perspective-correct barycentrics; -1 where nothing covers the
    pixel.  Indices are per mesh (every element behaves as a batch of one).  With a `scratch` the tensors are the scratch's
    own, overwritten by the next call that uses it.  Vertices that require grad are detached."""
    what = "rasterize_meshes"
    topo = _topology(what, faces)
    verts, key, scratch = _inputs(what, cameras, vertices, topo, scratch)
    with torch.no_grad():
        _rasterize(verts, cameras, topo, key, scratch)
    return Fragments(scratch.pix_to_face, scratch.zbuf, scratch.bary)


class Renderer:
    """recorder/mesh_renderer.py::Renderer: flat-shaded views (`forward`, `__call__`, batched: `render`) and the position /
    normal / depth / mask maps (`map`, batched: `maps`) of meshes that share a face list."""

    def __init__(self, white_background=True):
        self.white_background = bool(white_background)
        self._bg = (ctypes.c_float * 3)(*([1.0] * 3 if white_background else [0.0] * 3))
        self.image_size = None
        self._cached = None                                   # (faces tensor, its version, MeshTopology)

    def resize(self, H, W):
        """The image size the next calls must have (their cameras carry it; a mismatch raises ValueError)."""
        H, W = int(H), int(W)
        if not (1 <= H <= _lib.MESH_MAX_SIDE and 1 <= W <= _lib.MESH_MAX_SIDE):
            raise ValueError(f"Renderer.resize: image size {H} x {W} outside 1 .. {_lib.MESH_MAX_SIDE}")
        self.image_size = (H, W)

    def topology(self, faces):
        """The MeshTopology of a faces tensor, cached on the tensor (and its version counter)."""
        if isinstance(faces, MeshTopology):
            return faces
        if not torch.is_tensor(faces):
            return _topology("Renderer", faces)
        c = self._cached
        if c is None or c[0] is not faces or c[1] != faces._version:
            self._cached = c = (faces, faces._version, MeshTopology(faces))
        return c[2]

    def scratch(self, cameras, vertices, faces):
        """A MeshScratch for calls of this size."""
        topo = self.topology(faces)
        return MeshScratch(vertices.shape[0], vertices.shape[1], topo.F, cameras.H, cameras.W, device=vertices.device)

    def _prepare(self, what, cameras, vertices, faces, scratch):
        topo = self.topology(faces)
        if self.image_size is not None and isinstance(cameras, MeshCameras) and self.image_size != (cameras.H, cameras.W):
            raise ValueError(f"{what}: resized to {self.image_size}, the cameras render {(cameras.H, cameras.W)}")
        verts, key, scratch = _inputs(what, cameras, vertices, topo, scratch)
        return topo, verts, key, scratch

    def render(self, cameras, vertices, faces, verts_rgb=None, out=None, scratch=None):
        """-> (B,H,W,3) float32.  verts_rgb: (B,V,3), or (V,3) / (1,V,3) for every mesh; None: ones."""
        what = "Renderer.render"
        topo, verts, key, scratch = self._prepare(what, cameras, vertices, faces, scratch)
        B, V, F, H, W = key
        if verts_rgb is not None:
            if not torch.is_tensor(verts_rgb) or verts_rgb.dtype != torch.float32:
                raise ValueError(f"{what}: verts_rgb must be a float32 tensor")
            if verts_rgb.dim() == 2:
                verts_rgb = verts_rgb[None]
            if verts_rgb.dim() != 3 or tuple(verts_rgb.shape[1:]) != (V, 3) or verts_rgb.shape[0] not in (1, B):
                raise ValueError(f"{what}: expected verts_rgb ({B},{V},3) or ({V},3), got {tuple(verts_rgb.shape)}")
            _device(what, verts_rgb)
            verts_rgb = verts_rgb.detach().expand(B, V, 3).contiguous()
        image = _out(what, "out", out, (B, H, W, 3), verts.device)
        with torch.no_grad():
            _rasterize(verts, cameras, topo, key, scratch)
            check(_lib.lib().d3ga_mesh_shade_flat(B, V, F, H, W, dptr(verts), dptr(topo.faces(verts.device)), dptr(verts_rgb), dptr(cameras.data),
                                                  dptr(scratch.pix_to_face), dptr(scratch.bary), self._bg, dptr(image), stream_handle()),
                  "d3ga_mesh_shade_flat")
        return image

    def forward(self, cameras, vertices, faces, verts_rgb=None):
        """The reference's call: the (H,W,3) view of element 0."""
        return self.render(cameras, vertices, faces, verts_rgb)[0]

    __call__ = forward

    def maps(self, cameras, vertices, faces, out=None, scratch=None):
        """-> (position (B,H,W,3), normal (B,H,W,3), depth (B,H,W,1), mask (B,H,W,1)), float32, 0 at background pixels.
        out: a tuple of four such tensors."""
        what = "Renderer.maps"
        topo, verts, key, scratch = self._prepare(what, cameras, vertices, faces, scratch)
        B, V, F, H, W = key
        if out is not None and (not isinstance(out, (tuple, list)) or len(out) != 4):
            raise ValueError(f"{what}: out must be (position, normal, depth, mask)")
        names = (("position", 3), ("normal", 3), ("depth", 1), ("mask", 1))
        pos, nrm, depth, mask = (_out(what, n, None if out is None else out[k], (B, H, W, c), verts.device) for k, (n, c) in enumerate(names))
        offsets, lists = topo.csr(V, verts.device)
        L, s = _lib.lib(), stream_handle()
        with torch.no_grad():
            _rasterize(verts, cameras, topo, key, scratch)
            check(L.d3ga_mesh_vertex_normals(B, V, F, dptr(verts), dptr(topo.faces(verts.device)), dptr(offsets), dptr(lists), dptr(scratch.normals), s),
                  "d3ga_mesh_vertex_normals")
            check(L.d3ga_mesh_maps(B, V, F, H, W, dptr(verts), dptr(topo.faces(verts.device)), dptr(scratch.normals), dptr(cameras.data),
                                   dptr(scratch.pix_to_face), dptr(scratch.bary), dptr(pos), dptr(nrm), dptr(depth), dptr(mask), s),
                  "d3ga_mesh_maps")
        return pos, nrm, depth, mask

    def map(self, cameras, vertices, faces):
        """The reference's call: (position_map (H,W,3), normal_map (H,W,3), depth_map (H,W,1), mask (H,W,1)) of element 0."""
        return tuple(t[0] for t in self.maps(cameras, vertices, faces))


def vertex_normals(vertices, faces):
    """pytorch3d's verts_normals for (B,V,3) meshes that share a face list: (B,V,3), bit-reproducible (no atomics)."""
    what = "vertex_normals"
    topo = _topology(what, faces)
    if not torch.is_tensor(vertices) or vertices.dim() != 3 or vertices.shape[-1] != 3 or vertices.dtype != torch.float32:
        raise ValueError(f"{what}: expected float32 vertices (B,V,3)")
    B, V = vertices.shape[0], vertices.shape[1]
    if V < topo.min_verts:
        raise ValueError(f"{what}: the faces name vertex {topo.min_verts - 1}, the meshes have {V} vertices")
    _device(what, vertices)
    verts = vertices.detach().contiguous()
    offsets, lists = topo.csr(V, verts.device)
    out = torch.empty(B, V, 3, dtype=torch.float32, device=verts.device)
    with torch.no_grad():
        check(_lib.lib().d3ga_mesh_vertex_normals(B, V, topo.F, dptr(verts), dptr(topo.faces(verts.device)), dptr(offsets), dptr(lists), dptr(out),
                                                  stream_handle()), "d3ga_mesh_vertex_normals")
    return out


def interpolate_face_attributes(pix_to_face, barycentric_coords, face_attributes, out=None):
    """pytorch3d's `interpolate_face_attributes` as Renderer.map of the reference runs it (recorder/mesh_renderer.py:11,80-93):
    pix_to_face (N,H,W,K) int64 into the packed faces, < 0 at background pixels; barycentric_coords (N,H,W,K,3) float32;
    face_attributes (F,3,D) float32, 1 <= D <= 64 -> (N,H,W,K,D) float32: b0 a0 + b1 a1 + b2 a2 of the pixel's face, 0 at
    background pixels (and where an index is >= F).  The weights are taken as they come (the reference passes ones for its
    normal map).  FORWARD ONLY: inputs that require grad are detached.  Never synchronises with the host; with `out=` (a
    contiguous float32 tensor of the result's shape) nothing is allocated, so a captured step can contain it."""
    what = "interpolate_face_attributes"
    if not torch.is_tensor(pix_to_face) or pix_to_face.dim() != 4 or pix_to_face.dtype != torch.int64:
        raise ValueError(f"{what}: pix_to_face must be an int64 tensor (N,H,W,K)")
    if not torch.is_tensor(barycentric_coords) or tuple(barycentric_coords.shape) != tuple(pix_to_face.shape) + (3,) or \
            barycentric_coords.dtype != torch.float32:
        raise ValueError(f"{what}: barycentric_coords must be a float32 tensor {tuple(pix_to_face.shape) + (3,)}")
    if not torch.is_tensor(face_attributes) or face_attributes.dim() != 3 or face_attributes.shape[1] != 3 or \
            face_attributes.dtype != torch.float32:
        raise ValueError(f"{what}: face_attributes must be a float32 tensor (F,3,D)")
    F, D = int(face_attributes.shape[0]), int(face_attributes.shape[2])
    if not 1 <= D <= _lib.INTERP_MAX_D:
        raise ValueError(f"{what}: D = {D} outside 1 .. {_lib.INTERP_MAX_D}")
    _device(what, pix_to_face, barycentric_coords, face_attributes)
    p2f, bary, attrs = pix_to_face.detach().contiguous(), barycentric_coords.detach().contiguous(), face_attributes.detach().contiguous()
    res = _out(what, "out", out, tuple(pix_to_face.shape) + (D,), p2f.device)
    with torch.no_grad():
        check(_lib.lib().d3ga_interp_face_attrs(p2f.numel(), F, D, dptr(p2f), dptr(bary), dptr(attrs), dptr(res), stream_handle()),
              "d3ga_interp_face_attrs")
    return res
