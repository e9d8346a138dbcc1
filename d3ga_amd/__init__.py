"""d3ga_amd -- MI355X-native deform-and-rasterize hot path of D3GA.

Python host layer over libd3ga_hip.so (hand-written gfx950 HIP kernels behind the C ABI of include/d3ga.h).
There is NO CPU fallback: every op raises if the library is missing or the tensors are not on the GPU.
"""
from ._lib import D3GAError, lib, library_path  # noqa: F401
from .bary_interp import BaryBinding, bary_interp, cage_attr, mesh_means  # noqa: F401
from .evaluation import Evaluator, compute_errors, compute_heatmap, error_heatmap, psnr  # noqa: F401
from .frame_grid import GridWriter, Panel, compose_grid, compose_panels, to_uint8, write_text  # noqa: F401
from .frame_state import Embedding, FramePoses, RowCache, code_lookup, convert_optimizer_state  # noqa: F401
from .knn import knn_points  # noqa: F401
from .lpips import LPIPS  # noqa: F401
from .objective import TrainingObjective, scale_energy  # noqa: F401
from .pose_prior import PosePCA  # noqa: F401
from .mesh_render import (Fragments, MeshCameras, MeshScratch, MeshTopology, Renderer, interpolate_face_attributes,  # noqa: F401
                          rasterize_meshes, to_cameras, vertex_normals)
from .png import PngBuffer, encode_png, png_bytes, save_image  # noqa: F401
from .sample_prep import SamplePrep, prepare_actorshq, prepare_goliath  # noqa: F401
from .mesh_labels import FaceNeighbours, LabelTransfer, face_neighbours, grow_mask_region, majority_vote, median_filter_mesh  # noqa: F401
from .gauss_init import (SurfaceSamples, body_surface_draws, inflate, init_cage_parameters, sample_initial_points,  # noqa: F401
                         sample_surface, vertex_normals_angle)
from .template_bind import (CageBinding, LoopPlan, TemplateBinding, Unposed, beta_table, bind_body_template, bind_cage,  # noqa: F401
                            bind_cage_skin, loop_plan, loop_subdivide, nearest_vertex, star_pose, unpose)
from .cage_author import (Decimated, Smoothed, VoxelGrid, cage_processor, create_cage, decimate, face_components, fill_holes, isosurface,  # noqa: F401
                          keep_components, prepare, simplify, smooth_cage, smooth_improved, smooth_taubin, voxelize)
from .point_render import PCRenderer, PointFragments, PointScratch, rasterize_points  # noqa: F401

__all__ = ["D3GAError", "lib", "library_path", "Evaluator", "compute_errors", "compute_heatmap", "error_heatmap", "psnr", "LPIPS",
           "Fragments", "MeshCameras", "MeshScratch", "MeshTopology", "Renderer", "rasterize_meshes", "to_cameras", "vertex_normals",
           "PCRenderer", "PointFragments", "PointScratch", "rasterize_points", "knn_points", "interpolate_face_attributes",
           "BaryBinding", "bary_interp", "cage_attr", "mesh_means", "code_lookup", "Embedding", "RowCache", "FramePoses",
           "convert_optimizer_state", "scale_energy", "TrainingObjective", "PosePCA",
           "Panel", "compose_grid", "compose_panels", "to_uint8", "write_text", "GridWriter",
           "PngBuffer", "encode_png", "png_bytes", "save_image",
           "SamplePrep", "prepare_actorshq", "prepare_goliath",
           "FaceNeighbours", "LabelTransfer", "face_neighbours", "grow_mask_region", "majority_vote", "median_filter_mesh",
           "SurfaceSamples", "sample_surface", "vertex_normals_angle", "inflate", "body_surface_draws", "sample_initial_points",
           "init_cage_parameters",
           "LoopPlan", "loop_plan", "loop_subdivide", "beta_table", "nearest_vertex", "Unposed", "unpose", "star_pose", "TemplateBinding",
           "bind_body_template", "CageBinding", "bind_cage", "bind_cage_skin",
           "VoxelGrid", "Smoothed", "prepare", "voxelize", "fill_holes", "isosurface", "smooth_improved", "smooth_taubin", "face_components",
           "keep_components", "create_cage", "smooth_cage", "simplify", "cage_processor", "Decimated", "decimate"]
