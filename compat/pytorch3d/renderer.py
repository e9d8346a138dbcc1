"""pytorch3d.renderer for what the reference builds of it (recorder/mesh_renderer.py:12-21,30-49,66,77, recorder/pc_renderer.py:
12-18,25-30,66, lib/segmentation.py:23,38,57,84): the mesh view, the fragments and the point-cloud view, served by d3ga_amd's
HIP rasterizers (mesh_render.py, point_render.py).  Forward only.

The module-like classes are parameter-free nn.Modules, so `.cuda()` on the reference's wrappers passes through.  The known
departures of the renderers behind them carry over: a face with a vertex -- or a point -- at view
depth <= 0.01 is dropped, not clipped; the reference's `mask = pix_to_face > 0` loses the pixels of packed face 0; a covered
pixel of the point view is not blended with the background, so discs darken towards their rims."""
from collections import namedtuple

import torch
from torch import nn

__all__ = ["PerspectiveCameras", "Transform3d", "RasterizationSettings", "MeshRasterizer", "MeshRenderer", "HardFlatShader", "PointLights",
           "BlendParams", "TexturesVertex", "Fragments", "PointsRasterizationSettings", "PointsRasterizer", "PointsRenderer",
           "AlphaCompositor"]

Fragments = namedtuple("Fragments", ["pix_to_face", "zbuf", "bary_coords", "dists"])
PointFragments = namedtuple("PointFragments", ["idx", "zbuf", "dists"])


# ---- cameras -----------------------------------------------------------------------------------------------------------------
class Transform3d:
    """An affine map of points in pytorch3d's row-vector convention: X' = [X, 1] @ M for M (N,4,4)."""

    def __init__(self, matrix):
        self._matrix = matrix

    def get_matrix(self):
        return self._matrix

    def inverse(self):
        return Transform3d(torch.linalg.inv(self._matrix))

    def transform_points(self, points):
        """points (P,3) or (N,P,3) -> the same shape ((P,3) needs one transform)"""
        if points.dim() not in (2, 3) or points.shape[-1] != 3:
            raise ValueError(f"transform_points: expected (P,3) or (N,P,3), got {tuple(points.shape)}")
        M = self._matrix.to(points.dtype)
        batch = points if points.dim() == 3 else points[None]
        if batch.shape[0] not in (1, M.shape[0]) and M.shape[0] != 1:
            raise ValueError(f"transform_points: {batch.shape[0]} clouds but {M.shape[0]} transforms")
        out = batch @ M[:, :3, :3] + M[:, 3:4, :3]
        if points.dim() == 2:
            if out.shape[0] != 1:
                raise ValueError(f"transform_points: (P,3) points with {out.shape[0]} transforms")
            out = out[0]
        return out


def _flip_xy(t):
    return t * t.new_tensor([-1.0, -1.0, 1.0])


class PerspectiveCameras:
    """What `cameras_from_opencv_projection` returns: it keeps the OpenCV data (R, tvec, camera_matrix, image_size as (H, W)
    rows) and builds the MeshCameras the kernels read lazily, on first rasterization, so the object and its transforms work
    on CPU tensors.  View axes are pytorch3d's: +x left, +y up, +z forward."""

    def __init__(self, *args, **kwargs):
        opencv = kwargs.pop("_opencv", None)
        if opencv is None or args or kwargs:
            raise NotImplementedError("PerspectiveCameras: only cameras_from_opencv_projection(R, tvec, camera_matrix, image_size) "
                                      "is built (focal_length / principal_point / R / T constructors are not)")
        self.R_cv, self.tvec, self.camera_matrix, self.image_size = opencv
        self.device = self.R_cv.device
        self._mesh_cameras = {}

    def __len__(self):
        return self.R_cv.shape[0]

    def to(self, device):
        if torch.device(device) == self.device:
            return self
        return PerspectiveCameras(_opencv=tuple(t.to(device) for t in (self.R_cv, self.tvec, self.camera_matrix, self.image_size)))

    def cuda(self, device=None):
        return self.to("cuda" if device is None else device)

    def get_world_to_view_transform(self):
        """X_view = X_world @ R_p + T_p: R_p = R_cv^T with columns 0 and 1 negated, T_p = tvec with x and y negated."""
        N = len(self)
        R_p = _flip_xy(self.R_cv.transpose(1, 2))
        T_p = _flip_xy(self.tvec)
        M = torch.zeros(N, 4, 4, dtype=R_p.dtype, device=R_p.device)
        M[:, :3, :3] = R_p
        M[:, 3, :3] = T_p
        M[:, 3, 3] = 1.0
        return Transform3d(M)

    def get_camera_center(self):
        return self.get_world_to_view_transform().inverse().get_matrix()[:, 3, :3]

    def image_hw(self):
        """(H, W), one size for the batch (a host read of image_size, cached with the kernel cameras)"""
        if "hw" not in self._mesh_cameras:
            size = self.image_size.detach().cpu().reshape(-1, 2)
            if not bool((size == size[:1]).all()):
                raise NotImplementedError("PerspectiveCameras: image_size differs inside the batch")
            self._mesh_cameras["hw"] = (int(size[0, 0]), int(size[0, 1]))
        return self._mesh_cameras["hw"]

    def mesh_cameras(self, image_size, device):
        """The d3ga_amd.MeshCameras of these cameras for an (H, W) raster on `device`, built once per size."""
        from d3ga_amd.mesh_render import MeshCameras
        H, W = image_size
        if (H, W) != self.image_hw():
            raise NotImplementedError(f"raster_settings.image_size = {(H, W)} differs from the cameras' image_size = {self.image_hw()}: "
                                      "rendering at another resolution than the calibrated one is not built")
        key = (H, W, torch.device(device))
        if key not in self._mesh_cameras:
            self._mesh_cameras[key] = MeshCameras(self.R_cv, self.tvec, self.camera_matrix, (H, W), device=device)
        return self._mesh_cameras[key]


def _image_size(what, image_size):
    if isinstance(image_size, int):
        return (image_size, image_size)
    try:
        H, W = (int(v) for v in image_size)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: image_size must be an int or (H, W), got {image_size!r}") from None
    return (H, W)


def _cameras(what, cameras, own):
    cameras = own if cameras is None else cameras
    if not isinstance(cameras, PerspectiveCameras):
        raise ValueError(f"{what}: cameras must come from cameras_from_opencv_projection, got {type(cameras).__name__}")
    return cameras


# ---- the mesh view ----------------------------------------------------------------------------------------------------------------
class RasterizationSettings:
    """pytorch3d's keyword names; `image_size` stays assignable (Renderer.resize).  blur_radius != 0 and faces_per_pixel != 1 are
    refused when rasterizing; the bin-size arguments are accepted and ignored (the HIP rasterizer does not bin by face count)."""

    def __init__(self, image_size=256, blur_radius=0.0, faces_per_pixel=1, bin_size=None, max_faces_opengl=10_000_000,
                 max_faces_per_bin=None, perspective_correct=None, clip_barycentric_coords=None, cull_backfaces=False,
                 z_clip_value=None, cull_to_frustum=False):
        self.image_size, self.blur_radius, self.faces_per_pixel = image_size, blur_radius, faces_per_pixel
        self.bin_size, self.max_faces_opengl, self.max_faces_per_bin = bin_size, max_faces_opengl, max_faces_per_bin
        self.perspective_correct, self.clip_barycentric_coords = perspective_correct, clip_barycentric_coords
        self.cull_backfaces, self.z_clip_value, self.cull_to_frustum = cull_backfaces, z_clip_value, cull_to_frustum

    def _check(self):
        if self.blur_radius != 0:
            raise NotImplementedError(f"RasterizationSettings: blur_radius = {self.blur_radius!r}; only 0 is built")
        if self.faces_per_pixel != 1:
            raise NotImplementedError(f"RasterizationSettings: faces_per_pixel = {self.faces_per_pixel!r}; only 1 is built")
        if self.perspective_correct is False:
            raise NotImplementedError("RasterizationSettings: perspective_correct = False; the barycentrics are perspective-correct")
        for name in ("clip_barycentric_coords", "cull_backfaces", "cull_to_frustum"):
            if getattr(self, name):
                raise NotImplementedError(f"RasterizationSettings: {name} = {getattr(self, name)!r} is not built")
        if self.z_clip_value is not None:
            raise NotImplementedError("RasterizationSettings: z_clip_value is not built (faces at view depth <= 0.01 are dropped)")


def _mesh_inputs(what, meshes, cameras, settings):
    from .structures import Meshes
    if not isinstance(meshes, Meshes):
        raise ValueError(f"{what}: expected pytorch3d.structures.Meshes, got {type(meshes).__name__}")
    settings._check()
    verts = meshes.verts_padded().detach().float()
    return verts, meshes.topology(), cameras.mesh_cameras(_image_size(what, settings.image_size), verts.device)


class MeshRasterizer(nn.Module):
    """MeshRasterizer(raster_settings)(meshes, cameras=) -> Fragments(pix_to_face (N,H,W,1) int64 into the packed faces, -1 at
    background pixels; zbuf (N,H,W,1); bary_coords (N,H,W,1,3); dists None): d3ga_amd.rasterize_meshes."""

    def __init__(self, cameras=None, raster_settings=None):
        super().__init__()
        self.cameras = cameras
        self.raster_settings = RasterizationSettings() if raster_settings is None else raster_settings

    def forward(self, meshes, cameras=None, **kwargs):
        what = "MeshRasterizer"
        if kwargs:
            raise NotImplementedError(f"{what}: {sorted(kwargs)} are not built")
        from d3ga_amd.mesh_render import rasterize_meshes
        verts, topo, mc = _mesh_inputs(what, meshes, _cameras(what, cameras, self.cameras), self.raster_settings)
        frag = rasterize_meshes(mc, verts, topo)
        face = frag.pix_to_face.long()
        offset = torch.arange(verts.shape[0], device=verts.device, dtype=torch.int64)[:, None, None] * topo.F
        packed = torch.where(face >= 0, face + offset, face)
        return Fragments(packed[..., None], frag.zbuf[..., None], frag.bary_coords[:, :, :, None, :], None)


class TexturesVertex:
    """TexturesVertex(verts_features (N,V,3) or (1,V,3)): per-vertex colours of the flat shader."""

    def __init__(self, verts_features):
        if not torch.is_tensor(verts_features):
            raise NotImplementedError("TexturesVertex: verts_features as a list of tensors is not built")
        if verts_features.dim() != 3 or verts_features.shape[-1] != 3:
            raise ValueError(f"TexturesVertex: expected verts_features (N,V,3), got {tuple(verts_features.shape)}")
        self._features = verts_features

    def verts_features_padded(self):
        return self._features


def _triple(what, name, value, want):
    rows = torch.as_tensor(value, dtype=torch.float64).reshape(-1, 3)
    if not bool(((rows - want).abs() <= 1e-6).all()):
        raise NotImplementedError(f"{what}: {name} = {value!r}; the flat shader is built for ({want}, {want}, {want})")


class PointLights(nn.Module):
    """The reference's light (recorder/mesh_renderer.py:34-40): ambient 0.45, diffuse 0.35, specular 0.05 -- the constants of
    d3ga_mesh_shade_flat; other colours are refused.  `location` is assignable and not read: the light sits at the camera
    centre, where recorder/mesh_renderer.py:63-64 moves it before every call."""

    def __init__(self, ambient_color=((0.5, 0.5, 0.5),), diffuse_color=((0.3, 0.3, 0.3),), specular_color=((0.2, 0.2, 0.2),),
                 location=((0, 1, 0),), device="cpu"):
        super().__init__()
        what = "PointLights"
        _triple(what, "ambient_color", ambient_color, 0.45)
        _triple(what, "diffuse_color", diffuse_color, 0.35)
        _triple(what, "specular_color", specular_color, 0.05)
        self.ambient_color, self.diffuse_color, self.specular_color = ambient_color, diffuse_color, specular_color
        self.location = location


class BlendParams:
    """BlendParams(background_color=...): white or black (the two backgrounds d3ga_amd.Renderer is built with)."""

    def __init__(self, sigma=1e-4, gamma=1e-4, background_color=(1.0, 1.0, 1.0)):
        self.sigma, self.gamma, self.background_color = sigma, gamma, background_color
        self.white_background = _white("BlendParams", background_color)


def _white(what, color):
    c = [float(v) for v in (color.tolist() if torch.is_tensor(color) else color)]
    if c[:3] == [1.0, 1.0, 1.0] and len(c) in (3, 4):
        return True
    if c[:3] == [0.0, 0.0, 0.0] and len(c) in (3, 4):
        return False
    raise NotImplementedError(f"{what}: background_color = {color!r}; white and black are built")


class HardFlatShader(nn.Module):
    """HardFlatShader(device, lights, blend_params): holds the lights and the background; the shading is d3ga_mesh_shade_flat."""

    def __init__(self, device="cpu", cameras=None, lights=None, materials=None, blend_params=None):
        super().__init__()
        if materials is not None:
            raise NotImplementedError("HardFlatShader: materials is not built")
        if lights is None:
            raise NotImplementedError("HardFlatShader: lights = None (pytorch3d's default light) is not built; pass the PointLights")
        if not isinstance(lights, PointLights):
            raise NotImplementedError(f"HardFlatShader: lights must be PointLights, got {type(lights).__name__}")
        self.cameras, self.lights = cameras, lights
        self.blend_params = BlendParams() if blend_params is None else blend_params


class MeshRenderer(nn.Module):
    """MeshRenderer(rasterizer, shader)(meshes, cameras=) -> (N,H,W,4): RGB of d3ga_amd.Renderer.render (bit for bit), alpha 1 on
    covered pixels."""

    def __init__(self, rasterizer, shader):
        super().__init__()
        if not isinstance(rasterizer, MeshRasterizer) or not isinstance(shader, HardFlatShader):
            raise NotImplementedError("MeshRenderer: built for a MeshRasterizer with a HardFlatShader")
        self.rasterizer, self.shader = rasterizer, shader
        self._renderers = {}

    def forward(self, meshes, cameras=None, **kwargs):
        what = "MeshRenderer"
        if kwargs:
            raise NotImplementedError(f"{what}: {sorted(kwargs)} are not built")
        from d3ga_amd.mesh_render import Renderer
        cameras = _cameras(what, cameras, self.rasterizer.cameras)
        verts, topo, mc = _mesh_inputs(what, meshes, cameras, self.rasterizer.raster_settings)
        white = self.shader.blend_params.white_background
        if white not in self._renderers:
            self._renderers[white] = Renderer(white_background=white)
        renderer = self._renderers[white]
        rgb = None
        if meshes.textures is not None:
            if not isinstance(meshes.textures, TexturesVertex):
                raise NotImplementedError(f"{what}: textures must be TexturesVertex, got {type(meshes.textures).__name__}")
            rgb = meshes.textures.verts_features_padded().detach().float().to(verts.device)
        scratch = renderer.scratch(mc, verts, topo)
        image = renderer.render(mc, verts, topo, verts_rgb=rgb, scratch=scratch)
        alpha = (scratch.pix_to_face >= 0).to(image.dtype)[..., None]
        return torch.cat([image, alpha], dim=-1)


# ---- the point-cloud view -------------------------------------------------------------------------------------------------------
class PointsRasterizationSettings:
    """pytorch3d's keyword names; `image_size` stays assignable.  points_per_pixel <= 8; bin_size and max_points_per_bin are
    accepted and ignored (the HIP rasterizer bins by 16 x 16 tiles whatever the value)."""

    def __init__(self, image_size=256, radius=0.01, points_per_pixel=8, bin_size=None, max_points_per_bin=None):
        self.image_size, self.radius, self.points_per_pixel = image_size, radius, points_per_pixel
        self.bin_size, self.max_points_per_bin = bin_size, max_points_per_bin


def _point_inputs(what, point_clouds, cameras, settings):
    from .structures import Pointclouds
    if not isinstance(point_clouds, Pointclouds):
        raise ValueError(f"{what}: expected pytorch3d.structures.Pointclouds, got {type(point_clouds).__name__}")
    if torch.is_tensor(settings.radius):
        raise NotImplementedError(f"{what}: a radius per point is not built; pass one number")
    points = point_clouds.points_padded().detach().float()
    return points, cameras.mesh_cameras(_image_size(what, settings.image_size), points.device)


class PointsRasterizer(nn.Module):
    """PointsRasterizer(raster_settings)(point_clouds, cameras=) -> PointFragments(idx (N,H,W,K) int64 into the packed points, -1
    in empty slots; zbuf; dists): d3ga_amd.rasterize_points."""

    def __init__(self, cameras=None, raster_settings=None):
        super().__init__()
        self.cameras = cameras
        self.raster_settings = PointsRasterizationSettings() if raster_settings is None else raster_settings

    def forward(self, point_clouds, cameras=None, **kwargs):
        what = "PointsRasterizer"
        if kwargs:
            raise NotImplementedError(f"{what}: {sorted(kwargs)} are not built")
        from d3ga_amd.point_render import rasterize_points
        s = self.raster_settings
        points, mc = _point_inputs(what, point_clouds, _cameras(what, cameras, self.cameras), s)
        frag = rasterize_points(mc, points, radius=s.radius, points_per_pixel=s.points_per_pixel)
        idx = frag.idx.long()
        offset = torch.arange(points.shape[0], device=points.device, dtype=torch.int64)[:, None, None, None] * points.shape[1]
        return PointFragments(torch.where(idx >= 0, idx + offset, idx), frag.zbuf, frag.dists)


class AlphaCompositor(nn.Module):
    """AlphaCompositor(background_color): white or black; None is pytorch3d's "no background", i.e. black."""

    def __init__(self, background_color=None):
        super().__init__()
        self.background_color = background_color
        self.white_background = False if background_color is None else _white("AlphaCompositor", background_color)


class PointsRenderer(nn.Module):
    """PointsRenderer(rasterizer, compositor)(point_clouds, cameras=) -> (N,H,W,3): d3ga_amd.PCRenderer.render, bit for bit."""

    def __init__(self, rasterizer, compositor):
        super().__init__()
        if not isinstance(rasterizer, PointsRasterizer) or not isinstance(compositor, AlphaCompositor):
            raise NotImplementedError("PointsRenderer: built for a PointsRasterizer with an AlphaCompositor")
        self.rasterizer, self.compositor = rasterizer, compositor

    def forward(self, point_clouds, cameras=None, **kwargs):
        what = "PointsRenderer"
        if kwargs:
            raise NotImplementedError(f"{what}: {sorted(kwargs)} are not built")
        from d3ga_amd.point_render import PCRenderer
        s = self.rasterizer.raster_settings
        points, mc = _point_inputs(what, point_clouds, _cameras(what, cameras, self.rasterizer.cameras), s)
        colors = point_clouds.features_padded()
        if colors is not None:
            if colors.shape[-1] != 3:
                raise NotImplementedError(f"{what}: features with {colors.shape[-1]} channels; 3 are built")
            colors = colors.detach().float().to(points.device)
        renderer = PCRenderer(white_background=self.compositor.white_background, radius=s.radius, points_per_pixel=s.points_per_pixel)
        return renderer.render(mc, points, colors)
