"""The point-cloud view on the device: the reference's recorder/pc_renderer.py::PCRenderer.forward (a pytorch3d
PointsRasterizer that keeps the `points_per_pixel` nearest points of every pixel, + AlphaCompositor: the "3D Means" panel, every
Gaussian centre a small disc), without pytorch3d: a forward-only tile-binned rasterizer in HIP (csrc/point_raster.hip).  The
semantics are stated in DESIGN.md 4.4h; they are this library's specification of record (pytorch3d cannot be run next to it).

    cameras = PCRenderer.to_cameras(frame)            # the MeshCameras of mesh_render.to_cameras
    renderer = PCRenderer(white_background=True)      # radius 0.007, 5 points per pixel
    image = renderer(cameras, means3D)                # (H,W,3), element 0, as the reference returns it

`vertices` is (B,P,3) with one camera per element; `render` returns all B elements, `rasterize_points` the fragments.  There is
no backward: the reference only ever uses this view detached, and inputs that require grad are detached here.  GPU tensors
only.  No call synchronises with the host.  With `out=` and `scratch=` nothing is allocated, so a captured step can contain
`render`.

One quirk of the reference is kept: a covered pixel is not blended with the background, so discs darken towards their rims.
One departure: a point at view depth <= 0.01 is dropped (pytorch3d drops z < 0 only), as the mesh view drops such faces.
"""
import ctypes
import math
import operator
from collections import namedtuple

import torch

from . import _lib
from ._lib import D3GAError, check, dptr, require_cuda, stream_handle
from .mesh_render import MeshCameras, to_cameras

PointFragments = namedtuple("PointFragments", ["idx", "zbuf", "dists"])


class PointRenderDeviceError(D3GAError, ValueError):
    """A tensor that is not on the current GPU: a D3GAError as everywhere in this package, and a ValueError as every other
    argument error of this module."""


def _device(what, *tensors):
    try:
        require_cuda(*tensors)
    except D3GAError as e:
        raise PointRenderDeviceError(f"{what}: {e}") from None


def _settings(what, radius, points_per_pixel):
    try:
        radius = float(radius)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: radius must be a number, got {radius!r}") from None
    # the kernels read the radius as float32: the value they get must itself be positive and finite
    if not (math.isfinite(radius) and radius > 0 and 0 < ctypes.c_float(radius).value < math.inf):
        raise ValueError(f"{what}: radius must be positive and finite, got {radius!r}")
    try:
        K = None if isinstance(points_per_pixel, bool) else operator.index(points_per_pixel)
    except TypeError:
        K = None
    if K is None or not 1 <= K <= _lib.POINTS_MAX_K:
        raise ValueError(f"{what}: points_per_pixel must be an integer in 1 .. {_lib.POINTS_MAX_K}, got {points_per_pixel!r}")
    return radius, K


class PointScratch:
    """Everything `rasterize_points` and `PCRenderer.render` need besides their outputs, for one problem size and one pair of
    settings: the rasterizer's scratch (the per-tile lists) and the fragments.  Reusable from call to call (nothing in it needs
    to be clean), which is what a captured step wants."""

    def __init__(self, B, P, H, W, K, radius, device="cuda"):
        radius, K = _settings("PointScratch", radius, K)
        n = ctypes.c_size_t()
        check(_lib.lib().d3ga_points_raster_scratch_bytes(B, P, H, W, radius, ctypes.byref(n)), "d3ga_points_raster_scratch_bytes")
        self.key = (B, P, H, W, K, radius)
        self.raw = torch.empty(n.value, dtype=torch.uint8, device=device)
        self.idx = torch.empty(B, H, W, K, dtype=torch.int32, device=device)
        self.zbuf = torch.empty(B, H, W, K, dtype=torch.float32, device=device)
        self.dists = torch.empty(B, H, W, K, dtype=torch.float32, device=device)


def _inputs(what, cameras, vertices, K, radius, scratch):
    if not isinstance(cameras, MeshCameras):
        raise ValueError(f"{what}: cameras must be MeshCameras (to_cameras), got {type(cameras).__name__}")
    if not torch.is_tensor(vertices):
        raise ValueError(f"{what}: vertices must be a tensor, got {type(vertices).__name__}")
    if vertices.dim() != 3 or vertices.shape[-1] != 3:
        raise ValueError(f"{what}: expected vertices (B,P,3), got {tuple(vertices.shape)}")
    if vertices.dtype != torch.float32:
        raise ValueError(f"{what}: vertices must be float32, got {vertices.dtype}")
    B, P = vertices.shape[0], vertices.shape[1]
    if B != cameras.B:
        raise ValueError(f"{what}: {B} clouds but {cameras.B} cameras")
    if B * P >= 2 ** 31:
        raise ValueError(f"{what}: {B} x {P} points are more than the 2^31 - 1 accepted")
    _device(what, vertices, cameras.data)
    key = (B, P, cameras.H, cameras.W, K, radius)
    if scratch is None:
        scratch = PointScratch(*key, device=vertices.device)
    elif not isinstance(scratch, PointScratch) or scratch.key != key:
        raise ValueError(f"{what}: the scratch is for (B,P,H,W,K,radius) = {getattr(scratch, 'key', None)}, the call is {key}")
    elif scratch.raw.device != vertices.device:
        raise ValueError(f"{what}: the scratch is on {scratch.raw.device}, the vertices on {vertices.device}")
    return vertices.detach().contiguous(), key, scratch


def _rasterize(verts, cameras, key, scratch):
    B, P, H, W, K, radius = key
    check(_lib.lib().d3ga_points_rasterize(B, P, H, W, K, radius, dptr(verts), dptr(cameras.data), dptr(scratch.raw), dptr(scratch.idx),
                                           dptr(scratch.zbuf), dptr(scratch.dists), stream_handle()), "d3ga_points_rasterize")


def rasterize_points(cameras, vertices, radius=0.007, points_per_pixel=5, scratch=None):
    """-> PointFragments(idx (B,H,W,K) int32, zbuf (B,H,W,K), dists (B,H,W,K)): per pixel the K nearest points whose disc holds
    the pixel centre, nearest first (equal depths: the smaller index first): the index into the cloud, the view depth and the
    squared NDC distance; -1 in the empty slots.  Indices are per cloud (every element behaves as a batch of one).  With a
    `scratch` the tensors are the scratch's own, overwritten by the next call that uses it.  Vertices that require grad are
    detached."""
    what = "rasterize_points"
    radius, K = _settings(what, radius, points_per_pixel)
    verts, key, scratch = _inputs(what, cameras, vertices, K, radius, scratch)
    with torch.no_grad():
        _rasterize(verts, cameras, key, scratch)
    return PointFragments(scratch.idx, scratch.zbuf, scratch.dists)


class PCRenderer:
    """recorder/pc_renderer.py::PCRenderer: the point-cloud view (`forward`, `__call__`, batched: `render`)."""

    DEFAULT_COLOR = (154 / 255, 205 / 255, 50 / 255)
    to_cameras = staticmethod(to_cameras)

    def __init__(self, white_background=True, radius=0.007, points_per_pixel=5):
        self.radius, self.points_per_pixel = _settings("PCRenderer", radius, points_per_pixel)
        self.white_background = bool(white_background)
        self._bg = (ctypes.c_float * 3)(*([1.0] * 3 if white_background else [0.0] * 3))
        self.image_size = None

    def cuda(self, device=None):
        """The reference builds `PCRenderer(...).cuda()`: there is nothing to move, the call returns the renderer."""
        return self

    def resize(self, H, W):
        """The image size the next calls must have (their cameras carry it; a mismatch raises ValueError)."""
        H, W = int(H), int(W)
        if not (1 <= H <= _lib.MESH_MAX_SIDE and 1 <= W <= _lib.MESH_MAX_SIDE):
            raise ValueError(f"PCRenderer.resize: image size {H} x {W} outside 1 .. {_lib.MESH_MAX_SIDE}")
        self.image_size = (H, W)

    def scratch(self, cameras, vertices):
        """A PointScratch for calls of this size."""
        return PointScratch(vertices.shape[0], vertices.shape[1], cameras.H, cameras.W, self.points_per_pixel, self.radius,
                            device=vertices.device)

    def _prepare(self, what, cameras, vertices, scratch):
        if self.image_size is not None and isinstance(cameras, MeshCameras) and self.image_size != (cameras.H, cameras.W):
            raise ValueError(f"{what}: resized to {self.image_size}, the cameras render {(cameras.H, cameras.W)}")
        return _inputs(what, cameras, vertices, self.points_per_pixel, self.radius, scratch)

    def rasterize_points(self, cameras, vertices, scratch=None):
        """`rasterize_points` with this renderer's radius and points per pixel."""
        what = "PCRenderer.rasterize_points"
        verts, key, scratch = self._prepare(what, cameras, vertices, scratch)
        with torch.no_grad():
            _rasterize(verts, cameras, key, scratch)
        return PointFragments(scratch.idx, scratch.zbuf, scratch.dists)

    def render(self, cameras, vertices, colors=None, out=None, scratch=None):
        """-> (B,H,W,3) float32.  colors: (B,P,3), or (P,3) / (1,P,3) for every cloud; None: (154, 205, 50) / 255."""
        what = "PCRenderer.render"
        verts, key, scratch = self._prepare(what, cameras, vertices, scratch)
        B, P, H, W, K, radius = key
        if colors is not None:
            if not torch.is_tensor(colors) or colors.dtype != torch.float32:
                raise ValueError(f"{what}: colors must be a float32 tensor")
            if colors.dim() == 2:
                colors = colors[None]
            if colors.dim() != 3 or tuple(colors.shape[1:]) != (P, 3) or colors.shape[0] not in (1, B):
                raise ValueError(f"{what}: expected colors ({B},{P},3) or ({P},3), got {tuple(colors.shape)}")
            _device(what, colors)
            colors = colors.detach().expand(B, P, 3).contiguous()
        if out is None:
            image = torch.empty((B, H, W, 3), dtype=torch.float32, device=verts.device)
        elif not torch.is_tensor(out) or tuple(out.shape) != (B, H, W, 3) or out.dtype != torch.float32 or not out.is_contiguous() or \
                out.device != verts.device:
            raise ValueError(f"{what}: out must be a contiguous float32 tensor {(B, H, W, 3)} on {verts.device}")
        else:
            image = out
        with torch.no_grad():
            _rasterize(verts, cameras, key, scratch)
            check(_lib.lib().d3ga_points_composite(B, P, H, W, K, radius, dptr(scratch.idx), dptr(scratch.dists), dptr(colors), self._bg,
                                                   dptr(image), stream_handle()), "d3ga_points_composite")
        return image

    def forward(self, cameras, vertices, colors=None):
        """The reference's call: the (H,W,3) view of element 0."""
        return self.render(cameras, vertices, colors)[0]

    __call__ = forward
