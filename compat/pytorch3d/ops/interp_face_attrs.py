"""pytorch3d.ops.interp_face_attrs.interpolate_face_attributes (recorder/mesh_renderer.py:11,80-93): d3ga_interp_face_attrs."""
from d3ga_amd.mesh_render import interpolate_face_attributes  # noqa: F401

__all__ = ["interpolate_face_attributes"]
