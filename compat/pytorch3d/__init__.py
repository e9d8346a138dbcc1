"""Drop-in `pytorch3d` package surface for what the reference uses of it, served by d3ga_amd's HIP kernels (pytorch3d has no
ROCm build).  Exactly the names the reference imports, for exactly the ways it uses them; anything outside that raises
NotImplementedError with the argument named.  Importable without a GPU and without the built library.

    models/cage_net.py:21            from pytorch3d.ops import knn_points
    recorder/mesh_renderer.py:7-21   import pytorch3d; ops.interp_face_attrs.interpolate_face_attributes; renderer.{RasterizationSettings,
                                     MeshRenderer, MeshRasterizer, HardFlatShader, TexturesVertex, PointLights, PerspectiveCameras, BlendParams}
    recorder/pc_renderer.py:10-19    utils.cameras_from_opencv_projection; structures.Pointclouds; renderer.{PointsRasterizationSettings,
                                     PointsRasterizer, PerspectiveCameras, PointsRenderer, AlphaCompositor}; common.compat.meshgrid_ij
    lib/segmentation.py:21-23        utils.cameras_from_opencv_projection; structures.Meshes; renderer.{RasterizationSettings, MeshRasterizer,
                                     PerspectiveCameras}
    lib/cage.py:18, lib/batch.py:18  transforms.matrix_to_quaternion
    models/garment_net.py:11,187, models/mesh_net.py:23     import pytorch3d (pytorch3d.transforms.matrix_to_quaternion)
    utils/graphics_utils.py:13       ops.points_normals.estimate_pointcloud_normals (importable; it has no caller)
    datasets/goliath_dataset.py:28   io.{load_ply, save_ply}

`import pytorch3d` alone makes every submodule reachable as an attribute (recorder/mesh_renderer.py:61 and
models/garment_net.py:187 rely on that).  Semantics and departures: DESIGN.md 4.4j."""
from . import common, io, ops, renderer, structures, transforms, utils  # noqa: F401

__version__ = "0.7.8+d3ga_amd"
__all__ = ["common", "io", "ops", "renderer", "structures", "transforms", "utils"]
