"""pytorch3d.ops: `knn_points` (models/cage_net.py:21,66) and `interpolate_face_attributes`, both HIP kernels of d3ga_amd,
forward only; `points_normals.estimate_pointcloud_normals` is importable and not built (it has no caller)."""
from d3ga_amd.knn import knn_points  # noqa: F401

from . import interp_face_attrs, points_normals  # noqa: F401
from .interp_face_attrs import interpolate_face_attributes  # noqa: F401
from .points_normals import estimate_pointcloud_normals  # noqa: F401

__all__ = ["knn_points", "interpolate_face_attributes", "estimate_pointcloud_normals"]
