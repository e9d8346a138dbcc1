"""ctypes binding of libd3ga_hip.so (include/d3ga.h).  Fails loudly when the library is absent."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# D3GA_LIB_PATH: a diagnostic build (D3GA_DIAG=... python d3ga_amd/csrc/build.py -> libd3ga_hip_diag.so); never set in production
_PATH = os.environ.get("D3GA_LIB_PATH") or os.path.join(_HERE, "libd3ga_hip.so")
_lib = None
ACC_STRIDE = 16          # D3GA_ACC_STRIDE (include/d3ga.h): floats per Gaussian in the screen-space gradient accumulator
# Bumped by every graph replay (graph.CapturedStep / CapturedCutStep): a replayed optimizer updates weights IN PLACE without
# touching their `_version`, so host-side caches keyed by (data_ptr, _version) -- the packed weight panels of mlp.py --
# carry this epoch in their key as well (eager forward -> replays with in-graph Adam -> eager forward used stale panels).
replay_epoch = [0]
ABI_VERSION = 112       # D3GA_VERSION (include/d3ga.h)
# D3GA_KNOB_* (include/d3ga.h), in key order
KNOBS = ("composite_variant", "merge_slots", "tile_assign", "bwd_split", "sort_merge", "ssim_impl", "wgrad_ws", "chain_abl", "chain_grid")
CAMERA_SLOT_WINDOWED = -1.0    # D3GA_CAMERA_SLOT_WINDOWED (include/d3ga.h): tanfovx of a windowed camera slot, 9 floats per view in campos
LOSS_PARTIALS = 2048     # D3GA_LOSS_PARTIALS (include/d3ga.h): floats of scratch behind a two-stage loss reduction
BLUR_PARTIALS = 6144     # D3GA_BLUR_PARTIALS (include/d3ga.h): floats of scratch behind d3ga_blur_mix_bwd's three sums
CALIB_PARTIALS = 12288   # D3GA_CALIB_PARTIALS (include/d3ga.h): floats of scratch behind d3ga_color_calib_bwd's six sums per view
# D3GA_FRAME_* (include/d3ga.h): flags of d3ga_frame_prep
FRAME_GAMMA, FRAME_BG_WHITE, FRAME_ERODE_MASK, FRAME_CLOSE_HOLES, FRAME_IMAGE_U8, FRAME_SEG_F32 = 1, 2, 4, 8, 16, 32
# D3GA_EVAL_* (include/d3ga.h): flags of d3ga_eval_frames
EVAL_BG_WHITE, EVAL_COMPOSED, EVAL_ALPHA3, EVAL_BOUNDARY_F32 = 1, 2, 4, 8
EVAL_MAX_PARTIALS = 2048  # D3GA_EVAL_MAX_PARTIALS: d3ga_eval_partials(H, W) never exceeds it
MESH_MAX_SIDE = 16384    # D3GA_MESH_MAX_SIDE (include/d3ga.h): the largest frame side the mesh rasterizer accepts
MESH_CAM_FLOATS = 16     # D3GA_MESH_CAM_FLOATS: R row-major, t, fx, fy, cx, cy
INTERP_MAX_D = 64        # D3GA_INTERP_MAX_D: the most channels d3ga_interp_face_attrs interpolates
KNN_MAX_K = 16           # D3GA_KNN_MAX_K: the most neighbours d3ga_knn_points keeps per query
POINTS_MAX_K = 8       # D3GA_POINTS_MAX_K: the most points the point-cloud rasterizer keeps per pixel
LPIPS_PARTIALS = 1024   # D3GA_LPIPS_PARTIALS (include/d3ga.h): floats of scratch per image behind d3ga_lpips_tap's spatial mean
OPTIM_CHUNK = 8192     # D3GA_OPTIM_CHUNK (include/d3ga.h): elements per record of the optimizer's chunk table
OPTIM_ALIGNED16 = 1      # D3GA_OPTIM_ALIGNED16: flag of a chunk whose four pointers are 16-byte aligned


class D3GAError(RuntimeError):
    pass


def library_path():
    return _PATH


class RasterParams(ctypes.Structure):
    """struct d3ga_raster_params (include/d3ga.h)."""
    _fields_ = [("P", ctypes.c_int32), ("M", ctypes.c_int32), ("sh_degree", ctypes.c_int32),
                ("W", ctypes.c_int32), ("H", ctypes.c_int32),
                ("tanfovx", ctypes.c_float), ("tanfovy", ctypes.c_float), ("scale_modifier", ctypes.c_float),
                ("antialiasing", ctypes.c_int32), ("prefiltered", ctypes.c_int32), ("debug", ctypes.c_int32),
                ("opacity_activation", ctypes.c_int32), ("forward_only", ctypes.c_int32),
                ("acc_self_clearing", ctypes.c_int32), ("n_views", ctypes.c_int32), ("per_view_geometry", ctypes.c_int32),
                ("tile_cull", ctypes.c_int32),
                ("factor_rows", ctypes.c_int32), ("per_view_appearance", ctypes.c_int32), ("per_view_background", ctypes.c_int32)]


BODY_MAX_JOINTS = 64     # D3GA_BODY_MAX_JOINTS (include/d3ga.h)
BODY_MAX_SHAPE = 32      # D3GA_BODY_MAX_SHAPE: shape + expression coefficients
BODY_LD_ALIGN = 2048     # D3GA_BODY_LD_ALIGN: row stride alignment of the blend directions, in floats


def body_saved_floats(J):
    """D3GA_BODY_SAVED_FLOATS(J): floats per frame of the body model forward's `saved` buffer."""
    return 27 * J + 16


class BodyModel(ctypes.Structure):
    """struct d3ga_body_model (include/d3ga.h): sizes and device pointers of a prepared SMPL / SMPL-X model."""
    _fields_ = [("V", ctypes.c_int32), ("J", ctypes.c_int32), ("n_shape", ctypes.c_int32), ("n_expr", ctypes.c_int32),
                ("n_hand_pca", ctypes.c_int32), ("ld", ctypes.c_int32), ("n_levels", ctypes.c_int32), ("reserved", ctypes.c_int32)] + \
               [(n, ctypes.c_void_p) for n in ("v_template", "dirs", "w_ptr", "w_joint", "w_val", "wt_ptr", "wt_vert", "wt_val",
                                               "J0", "Jdirs", "parents", "level_ptr", "level_joint", "child_ptr", "child_joint",
                                               "hand_comps", "hand_mean")]


class LbsPoseGrad(ctypes.Structure):
    """struct d3ga_lbs_pose_grad (include/d3ga.h): the by-joint plan, scratch and outputs of the D0 pose backward."""
    _fields_ = [("J", ctypes.c_int32), ("n_chunks", ctypes.c_int32), ("n_entries", ctypes.c_int64)] + \
               [(n, ctypes.c_void_p) for n in ("tmpl", "delta", "chunk_ptr", "chunk_range", "entries", "counter", "scratch", "g_joint_mats",
                                               "g_Rh", "g_Th")]


DEFORM_ROUTE_CORNERS, DEFORM_ROUTE_MERGE = 1, 2    # D3GA_DEFORM_ROUTE_* (include/d3ga.h)


class CageDeformIn(ctypes.Structure):
    """struct d3ga_cage_deform_in (include/d3ga.h): sizes, flags and inputs of the fused cage deformation."""
    _fields_ = [(n, ctypes.c_int32) for n in ("P", "V", "flags", "reserved")] + \
               [(n, ctypes.c_void_p) for n in ("tetpoints", "tetras", "tetra_id", "barys", "canon_grad", "scales", "rots", "delta_barys")]


class CageDeformGrads(ctypes.Structure):
    """struct d3ga_cage_deform_grads: the two incoming and the four outgoing gradients of its backward."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("g_means", "g_cov6", "g_tetpoints", "g_barys", "g_scales", "g_rots")]


class CageDeformRoute(ctypes.Structure):
    """struct d3ga_cage_deform_route: how the backward sums the vertex gradient (per-corner records | block-merge plan)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("kind", "n_segments")] + \
               [(n, ctypes.c_void_p) for n in ("item_pos", "seg_begin", "seg_ptr", "vert_start", "vert_items", "records")]


class CageDeformSkin(ctypes.Structure):
    """struct d3ga_cage_deform_skin: the skinning backward in the vertex-gather launch of the merge route."""
    _fields_ = [(n, ctypes.c_int32) for n in ("K", "reserved")] + \
               [(n, ctypes.c_void_p) for n in ("joint_mats", "skin_idx", "skin_w", "Rh", "g_tetpoints_extra", "g_delta")]


SKEL_MAX_JOINTS = 512    # D3GA_SKEL_MAX_JOINTS (include/d3ga.h)
SKEL_SAVED_FLOATS = 12   # D3GA_SKEL_SAVED_FLOATS: floats per joint of the skeleton forward's `saved` buffer


class Skeleton(ctypes.Structure):
    """struct d3ga_skeleton (include/d3ga.h): sizes and device pointers of a prepared Goliath skeleton."""
    _fields_ = [("J", ctypes.c_int32), ("n_params", ctypes.c_int32), ("n_levels", ctypes.c_int32), ("n_children", ctypes.c_int32)] + \
               [(n, ctypes.c_void_p) for n in ("parents", "level_ptr", "level_joint", "child_ptr", "child_joint", "joint_offset",
                                               "joint_rotation", "transform_offsets", "csr_ptr", "csr_col", "csr_val", "csc_ptr",
                                               "csc_row", "csc_val")]


CODE_MAX_B, CODE_MAX_D = 16, 4096    # D3GA_CODE_MAX_B, D3GA_CODE_MAX_D (include/d3ga.h): indices per lookup, widest code row
ROW_CACHE_MAX_PAIRS = 16             # D3GA_ROW_CACHE_MAX_PAIRS: (table, stage) pairs of one d3ga_row_cache_select


class RowPair(ctypes.Structure):
    """struct d3ga_row_pair (include/d3ga.h): a table (n_rows, width) and its staged row, 4-byte words."""
    _fields_ = [("table", ctypes.c_void_p), ("stage", ctypes.c_void_p), ("width", ctypes.c_int32), ("n_rows", ctypes.c_int32)]


SCALE_ACT_NONE, SCALE_ACT_EXP = 0, 1     # D3GA_SCALE_ACT_* (include/d3ga.h)
SCALE_ENERGY_GRID = 1536                 # D3GA_SCALE_ENERGY_GRID: workgroups (256 threads x 4 floats) of scale_energy's first stage, at most
OBJ_MAX_FRAMES, OBJ_SLOTS, OBJ_MAX_LEN, OBJ_TERMS = 16, 9, 4096, 9    # D3GA_OBJ_* (include/d3ga.h)
OBJ_STATUS_NAN_SEEN, OBJ_STATUS_FIRST_BAD, OBJ_STATUS_STEPS, OBJ_STATUS_TERMS, OBJ_STATUS_WORDS = 0, 1, 2, 4, 16


POSE_MAX_D, POSE_FIT_CHUNK = 256, 256    # D3GA_POSE_MAX_D, D3GA_POSE_FIT_CHUNK (include/d3ga.h): widest pose / most components, rows per reduction chunk of the fit
POSE_STAGE_PROJECT, POSE_STAGE_CLIP, POSE_STAGE_RECONSTRUCT = 1, 2, 4    # D3GA_POSE_STAGE_*: stages of d3ga_pose_clamp


GRID_MAX_PANELS, GRID_MAX_LABEL, GRID_MAX_SIDE = 16, 64, 32768    # D3GA_GRID_MAX_* (include/d3ga.h)
GRID_OUT_F32_CHW, GRID_OUT_F32_HWC, GRID_OUT_U8_SAVE_IMAGE, GRID_OUT_U8_CLIP = 0, 1, 2, 3    # D3GA_GRID_OUT_*: modes of d3ga_frame_grid
GRID_BGR, GRID_FORCE_SCALAR = 1, 2       # D3GA_GRID_*: flags of the grid
PANEL_BOTTOM, PANEL_BOLD = 1, 2          # D3GA_PANEL_*: flags of a panel
PNG_FILTER_ADAPTIVE = 5                  # D3GA_PNG_FILTER_ADAPTIVE: filter argument of d3ga_png_encode (0..4 force a type)
LABELS_MAX, LABEL_RINGS_MAX = 32, 4096   # D3GA_LABELS_MAX, D3GA_LABEL_RINGS_MAX (include/d3ga.h): columns of a label histogram, rings of one growth call
LABEL_EVERY_PIXEL = 1                    # D3GA_LABEL_EVERY_PIXEL: flag of d3ga_label_vote (measurement only)
LABEL_STATUS_RANGE = 1                   # D3GA_LABEL_STATUS_RANGE: bit of the vote's status word
SAMPLE_MAX_FACES = 1 << 24               # D3GA_SAMPLE_MAX_FACES (include/d3ga.h): d3ga_surface_sample takes fewer faces than this
SAMPLE_STATUS_EMPTY, SAMPLE_STATUS_RANGE = 1, 2    # D3GA_SAMPLE_STATUS_*: bits of the surface sampler's status word
BIND_STATUS_RANGE, BIND_STATUS_NONMANIFOLD, BIND_STATUS_DEGENERATE, BIND_STATUS_SINGULAR = 1, 2, 4, 8    # D3GA_BIND_STATUS_*: template binding
LOOP_BAD_KEY = 2 ** 63 - 1                         # D3GA_LOOP_BAD_KEY: the key of a face that takes no part in a Loop plan


class LoopPlanTables(ctypes.Structure):
    """struct d3ga_loop_plan (include/d3ga.h): sizes and device tables of one level of Loop subdivision."""
    _fields_ = [(n, ctypes.c_int32) for n in ("V", "F", "E", "reserved")] + \
               [(n, ctypes.c_void_p) for n in ("edge_verts", "edge_opp", "edge_faces", "edge_boundary", "face_edge", "vert_offsets",
                                               "vert_nbr", "vert_boundary")]


CAGE_MAX_RADIUS, CAGE_MAX_ITERATIONS = 511, 4096   # D3GA_CAGE_MAX_* (include/d3ga.h): cage surface authoring
CAGE_STATUS_RANGE, CAGE_STATUS_ISOLATED, CAGE_STATUS_ZERO_EDGE = 1, 2, 4    # D3GA_CAGE_STATUS_*: bits of its status words
CAGE_FILL_BEGIN, CAGE_FILL_ROUND, CAGE_FILL_FINISH = 0, 1, 2               # D3GA_CAGE_FILL_*: stages of d3ga_cage_fill
CAGE_SMOOTH_IMPROVED, CAGE_SMOOTH_TAUBIN = 0, 1                            # D3GA_CAGE_SMOOTH_*: modes of d3ga_cage_smooth
CAGE_PARTS_BEGIN, CAGE_PARTS_ROUND = 0, 1                                  # D3GA_CAGE_PARTS_*: stages of d3ga_cage_components
CAGE_STATUS_STUCK = 8                                                      # D3GA_CAGE_STATUS_STUCK: decimation ended above its target


class VoxelGridDesc(ctypes.Structure):
    """struct d3ga_voxel_grid (include/d3ga.h): a bit-packed occupancy grid of (2 radius + 1)^3 voxels."""
    _fields_ = [(n, ctypes.c_int32) for n in ("radius", "D", "W", "reserved")] + [("bits", ctypes.c_void_p)]


class CageIsoDesc(ctypes.Structure):
    """struct d3ga_cage_iso_desc (include/d3ga.h): where the isosurface goes and how grid coordinates map to it."""
    _fields_ = [("n_vertices", ctypes.c_int32), ("n_faces", ctypes.c_int32), ("centre", ctypes.c_double * 3), ("scale", ctypes.c_double * 3),
                ("vertices", ctypes.c_void_p), ("faces", ctypes.c_void_p)]


class CageSmoothDesc(ctypes.Structure):
    """struct d3ga_cage_smooth_desc (include/d3ga.h): one run of a smoother."""
    _fields_ = [("mode", ctypes.c_int32), ("iterations", ctypes.c_int32), ("lam", ctypes.c_double), ("mu", ctypes.c_double)] + \
               [(n, ctypes.c_void_p) for n in ("x", "work", "normals", "faces", "csr_offsets", "csr_faces", "out", "status")]


class DecimateDesc(ctypes.Structure):
    """struct d3ga_decimate_desc (include/d3ga.h): the state and the per-round tables of quadric decimation."""
    _fields_ = [("n_admit", ctypes.c_int32), ("reserved", ctypes.c_int32)] + \
               [(n, ctypes.c_void_p) for n in ("x", "quadrics", "faces", "csr_offsets", "csr_faces", "keys", "placement", "sorted_keys", "owner",
                                               "remap", "faces_out", "scratch")] + \
               [("scratch_bytes", ctypes.c_int64), ("counts", ctypes.c_void_p), ("status", ctypes.c_void_p)]


class GridPanel(ctypes.Structure):
    """struct d3ga_grid_panel (include/d3ga.h): a source view, where it goes on the canvas, and its label."""
    _fields_ = [("src", ctypes.c_void_p), ("value", ctypes.c_void_p), ("sc", ctypes.c_int64), ("sh", ctypes.c_int64),
                ("sw", ctypes.c_int64)] + \
               [(n, ctypes.c_int32) for n in ("C", "h", "w", "y0", "x0", "flags", "label_len", "X")] + \
               [("color", ctypes.c_float * 3), ("label", ctypes.c_char * GRID_MAX_LABEL)]


class GridDesc(ctypes.Structure):
    """struct d3ga_grid_desc (include/d3ga.h): the canvas, the output mode and the panel table."""
    _fields_ = [(n, ctypes.c_int32) for n in ("n_panels", "out_H", "out_W", "mode", "channels", "flags")] + \
               [("pad_value", ctypes.c_float), ("reserved", ctypes.c_int32), ("pitch", ctypes.c_int64),
                ("panel", GridPanel * GRID_MAX_PANELS)]


class ObjectiveEntry(ctypes.Structure):
    """struct d3ga_objective_entry (include/d3ga.h): one input of one frame, and where its gradient goes."""
    _fields_ = [("ptr", ctypes.c_void_p), ("len", ctypes.c_int32), ("goff", ctypes.c_int32)]


class ObjectiveDesc(ctypes.Structure):
    """struct d3ga_objective_desc (include/d3ga.h): the weights and the frame-major table of entries."""
    _fields_ = [("n_frames", ctypes.c_int32), ("reserved", ctypes.c_int32)] + \
               [(n, ctypes.c_float) for n in ("lambda_dssim", "rgb_weight", "sil_weight", "fme_weight", "blur_weight", "vgg_weight")] + \
               [("entry", ObjectiveEntry * (OBJ_MAX_FRAMES * OBJ_SLOTS))]


_vp, _i, _i64, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
_prm = ctypes.POINTER(RasterParams)
_bm = ctypes.POINTER(BodyModel)
_lpg = ctypes.POINTER(LbsPoseGrad)
_sk = ctypes.POINTER(Skeleton)

# what the *_deform entries take behind their parent's arguments: the deform backward that runs as the per-Gaussian kernel's tail
_deform_tail = [ctypes.POINTER(c) for c in (CageDeformIn, CageDeformGrads, CageDeformRoute)]

# name -> (argtypes, restype); the trailing _vp of every launch entry is the hipStream_t
_SIGNATURES = {
    "d3ga_version": ([], _i),
    "d3ga_status_string": ([_i], ctypes.c_char_p),
    "d3ga_debug_set": ([ctypes.c_int32, ctypes.c_int32], _i),
    "d3ga_debug_defaults": ([ctypes.POINTER(ctypes.c_int32), ctypes.c_int32], _i),
    "d3ga_lbs_cage_fwd": ([_i, _i] + [_vp] * 8 + [_vp], _i),
    "d3ga_lbs_cage_bwd": ([_i, _i] + [_vp] * 6 + [_lpg, _vp], _i),
    "d3ga_lbs_pose_scratch_bytes": ([_i, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_i64)], _i),
    "d3ga_cage_deform_fwd": ([ctypes.POINTER(CageDeformIn), _vp, _vp, _vp], _i),
    "d3ga_cage_deform_bwd": ([ctypes.POINTER(c) for c in (CageDeformIn, CageDeformGrads, CageDeformRoute, CageDeformSkin)] + [_lpg, _vp], _i),
    "d3ga_cage_deform_bwd_tail": ([ctypes.POINTER(c) for c in (CageDeformIn, CageDeformGrads, CageDeformRoute, CageDeformSkin)] + [_lpg, _vp], _i),
    "d3ga_fem_energy_fwd": ([_i] + [_vp] * 4 + [_vp], _i),
    "d3ga_fem_energy_bwd": ([_i, _i] + [_vp] * 5 + [_vp], _i),
    "d3ga_bary_interp_fwd": ([ctypes.c_int32] * 3 + [_vp] * 5 + [_vp], _i),
    "d3ga_bary_interp_bwd": ([ctypes.c_int32] * 4 + [_vp] * 9 + [_vp], _i),
    "d3ga_raster_scratch_bytes": ([ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _i64, ctypes.POINTER(_i64)], _i),
    "d3ga_raster_scratch_bytes_views": ([ctypes.c_int32] * 4 + [_i64, ctypes.c_int32, ctypes.POINTER(_i64)], _i),
    "d3ga_raster_scratch_bytes_window": ([ctypes.c_int32] * 4 + [_i64, ctypes.c_int32, ctypes.POINTER(_i64)], _i),
    "d3ga_raster_binning_layout_window": ([ctypes.c_int32] * 3 + [_i64, ctypes.POINTER(_i64)], _i),
    "d3ga_raster_binning_layout": ([ctypes.c_int32, ctypes.c_int32, _i64, ctypes.POINTER(_i64)], _i),
    "d3ga_raster_img_layout": ([ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_i64)], _i),
    "d3ga_raster_img_layout_blocks": ([ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_i64)], _i),
    "d3ga_raster_img_bytes": ([ctypes.c_int32, ctypes.c_int32, _i64, ctypes.c_int32], _i64),
    "d3ga_raster_preprocess": ([_prm] + [_vp] * 12 + [_i64, _vp, _vp], _i),
    "d3ga_raster_bin_sort": ([_prm, _vp, _vp, _i64, _vp], _i),
    "d3ga_raster_composite_fwd": ([_prm, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp], _i),
    "d3ga_raster_composite_bwd": ([_prm, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp], _i),
    "d3ga_raster_composite_bwd_depth": ([_prm, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp], _i),
    "d3ga_raster_composite_fwd2": ([_prm, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp], _i),
    "d3ga_raster_composite_bwd2": ([_prm, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp], _i),
    "d3ga_raster_preprocess_bwd": ([_prm] + [_vp] * 18 + [_vp], _i),
    "d3ga_raster_preprocess_bwd_deform": ([_prm] + [_vp] * 18 + _deform_tail + [_vp], _i),
    "d3ga_raster_forward": ([_prm] + [_vp] * 14 + [_i64, _vp, _vp, _vp, _vp], _i),
    "d3ga_raster_backward": ([_prm] + [_vp] * 11 + [_i64] + [_vp] * 11 + [_vp], _i),
    "d3ga_raster_backward_deform": ([_prm] + [_vp] * 11 + [_i64] + [_vp] * 11 + _deform_tail + [_vp], _i),
    "d3ga_raster_composite_fwd_l1": ([_prm, _vp, _vp, _vp, _i64] + [_vp] * 7 + [_vp], _i),
    "d3ga_raster_composite_bwd_l1": ([_prm, _vp, _vp, _vp, _i64] + [_vp] * 7 + [_vp], _i),
    "d3ga_raster_backward_l1": ([_prm] + [_vp] * 11 + [_i64] + [_vp] * 15 + [_vp], _i),
    "d3ga_raster_backward_l1_deform": ([_prm] + [_vp] * 11 + [_i64] + [_vp] * 15 + _deform_tail + [_vp], _i),
    "d3ga_raster_recolor": ([_prm] + [_vp] * 6 + [_vp], _i),
    "d3ga_raster_mark_visible": ([ctypes.c_int32, _vp, _vp, _vp, _vp], _i),
    "d3ga_sh_grad_from_views": ([ctypes.c_int32] * 4 + [_vp, _vp, _i64, _vp, _i64, ctypes.c_float, _vp, _vp], _i),
    "d3ga_compute_bary": ([_i, _i] + [_vp] * 5 + [_vp], _i),
    "d3ga_selftest_row_scan": ([_i, _vp, _vp, _vp], _i),
    "d3ga_selftest_alpha": ([ctypes.c_int32, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp], _i),
    "d3ga_knn3_mean_dist2": ([_i, _vp, _vp, _vp], _i),
    "d3ga_compute_bary_grid": ([_i] + [_vp] * 9 + [_vp], _i),
    "d3ga_knn3_mean_dist2_grid": ([_i] + [_vp] * 6 + [_vp], _i),
    "d3ga_knn_points": ([_i] * 4 + [_vp] * 4 + [_vp], _i),
    "d3ga_knn_points_grid": ([_i] * 3 + [_vp] * 8 + [_vp], _i),
    "d3ga_interp_face_attrs": ([_i64, _i64, _i] + [_vp] * 4 + [_vp], _i),
    "d3ga_l1_mean_fwd": ([_i64, _vp, _vp, _vp, _vp], _i),
    "d3ga_l1_mean_fwd_ws": ([_i64, _vp, _vp, _vp, _vp, _vp], _i),
    "d3ga_l1_mean_bwd": ([_i64, _vp, _vp, _vp, _vp, _vp], _i),
    "d3ga_l1_mean_fwd_ws_cell": ([_i64, _vp, _vp, _vp, _vp, _vp], _i),
    "d3ga_l1_mean_bwd_cell": ([_i64, _vp, _vp, _vp, _vp, _vp], _i),
    "d3ga_mlp_panel_bytes": ([ctypes.c_int32, ctypes.c_int32], _i64),
    "d3ga_mlp_pack_weights": ([ctypes.c_int32, ctypes.c_int32, _vp, _i64, _i64, _vp, _vp], _i),
    "d3ga_mlp_linear": ([ctypes.c_int32] * 3 + [_vp, _vp, _vp, ctypes.c_float, _vp, _vp, ctypes.c_float, _vp, _vp], _i),
    "d3ga_mlp_chain_panel_bytes": ([ctypes.c_int32, ctypes.c_int32], _i64),
    "d3ga_mlp_pack_chain": ([ctypes.c_int32, ctypes.c_int32, _vp, _i64, _i64, _vp, _vp], _i),
    "d3ga_mlp_chain_fwd": ([ctypes.c_int32, ctypes.c_int32, _vp, ctypes.c_int32] + [_vp] * 9 + [_vp], _i),
    "d3ga_mlp_wgrad": ([ctypes.c_int32] * 3 + [_vp] * 4 + [_vp], _i),
    "d3ga_mlp_wgrad_acc": ([ctypes.c_int32] * 3 + [_vp] * 4 + [_vp], _i),
    "d3ga_field_heads_fwd": ([ctypes.c_int32] * 3 + [_vp, _vp, _vp, _vp, _vp, _vp], _i),
    "d3ga_field_heads_bwd": ([ctypes.c_int32] * 3 + [_vp, _vp, _vp] + [_vp] * 6 + [_vp], _i),
    "d3ga_view_dirs_fwd": ([ctypes.c_int32, _vp, _vp, _vp, _vp], _i),
    "d3ga_view_dirs_bwd": ([ctypes.c_int32, _vp, _vp, _vp, _vp, _vp], _i),
    "d3ga_sh4_encoding_fwd": ([ctypes.c_int32, _vp, _vp, _vp], _i),
    "d3ga_sh4_encoding_bwd": ([ctypes.c_int32, _vp, _vp, _vp, _vp], _i),
    "d3ga_color_rows_fwd": ([ctypes.c_int32, ctypes.c_int32, _vp, _vp, _vp, _vp], _i),
    "d3ga_color_rows_bwd": ([ctypes.c_int32, ctypes.c_int32, _vp, _vp, _vp, _vp, _vp], _i),
    "d3ga_ssim_fwd": ([ctypes.c_int32] * 3 + [_vp] * 6 + [_vp], _i),
    "d3ga_ssim_bwd": ([ctypes.c_int32] * 3 + [_vp] * 7 + [_vp], _i),
    "d3ga_ssim_l1_fwd": ([ctypes.c_int32] * 3 + [_vp] * 7 + [_vp], _i),
    "d3ga_ssim_l1_bwd": ([ctypes.c_int32] * 3 + [_vp] * 8 + [_vp], _i),
    "d3ga_blur_mix_fwd": ([ctypes.c_int32] * 4 + [_vp] * 4 + [_vp], _i),
    "d3ga_blur_mix_bwd": ([ctypes.c_int32] * 4 + [_vp] * 7 + [_vp], _i),
    "d3ga_compose_target": ([ctypes.c_int32] * 3 + [_vp] * 4 + [ctypes.c_int32] + [_vp] * 3 + [_vp], _i),
    "d3ga_color_calib_fwd": ([ctypes.c_int32] * 5 + [_vp] * 4 + [_vp], _i),
    "d3ga_color_calib_bwd": ([ctypes.c_int32] * 5 + [_f] + [_vp] * 7 + [_vp], _i),
    "d3ga_pixel_bias_fwd": ([ctypes.c_int32] * 6 + [_vp] * 4 + [_vp], _i),
    "d3ga_pixel_bias_bwd": ([ctypes.c_int32] * 6 + [_vp] * 3 + [_vp], _i),
    "d3ga_frame_prep": ([ctypes.c_int32] * 4 + [_vp] * 4 + [ctypes.c_int32] + [_vp] * 5 + [_vp], _i),
    "d3ga_eval_frames": ([ctypes.c_int32] * 4 + [_vp] * 8 + [_vp], _i),
    "d3ga_eval_finish": ([ctypes.c_int32] * 3 + [_vp] * 5 + [_vp], _i),
    "d3ga_eval_ssim": ([ctypes.c_int32] * 3 + [_vp] * 3 + [_vp], _i),
    "d3ga_eval_partials": ([ctypes.c_int32] * 2, _i64),
    "d3ga_eval_ssim_partials": ([ctypes.c_int32] * 2, _i64),
    "d3ga_eval_jet_table": ([_vp], _i),
    "d3ga_mesh_raster_scratch_bytes": ([ctypes.c_int32] * 5 + [ctypes.POINTER(ctypes.c_size_t)], _i),
    "d3ga_mesh_rasterize": ([ctypes.c_int32] * 5 + [_vp] * 7 + [_vp], _i),
    "d3ga_mesh_shade_flat": ([ctypes.c_int32] * 5 + [_vp] * 6 + [ctypes.POINTER(ctypes.c_float), _vp] + [_vp], _i),
    "d3ga_mesh_vertex_normals": ([ctypes.c_int32] * 3 + [_vp] * 5 + [_vp], _i),
    "d3ga_mesh_maps": ([ctypes.c_int32] * 5 + [_vp] * 10 + [_vp], _i),
    "d3ga_points_raster_scratch_bytes": ([ctypes.c_int32] * 4 + [_f, ctypes.POINTER(ctypes.c_size_t)], _i),
    "d3ga_points_rasterize": ([ctypes.c_int32] * 5 + [_f] + [_vp] * 6 + [_vp], _i),
    "d3ga_points_composite": ([ctypes.c_int32] * 5 + [_f] + [_vp] * 3 + [ctypes.POINTER(ctypes.c_float), _vp] + [_vp], _i),
    "d3ga_optim_scratch_bytes":([ctypes.c_int32] * 3 + [ctypes.POINTER(_i64)], _i),
    "d3ga_optim_clip_adam_step": ([_vp, ctypes.c_int32, _vp, ctypes.c_int32, _vp, ctypes.c_int32, ctypes.c_float, _vp, _vp, _vp], _i),
    "d3ga_body_model_scratch_bytes": ([_bm, ctypes.c_int32, ctypes.POINTER(_i64), ctypes.POINTER(_i64)], _i),
    "d3ga_body_model_fwd": ([_bm, ctypes.c_int32, ctypes.c_int32] + [_vp] * 10 + [_vp, _i64, _vp], _i),
    "d3ga_body_model_bwd": ([_bm, ctypes.c_int32, ctypes.c_int32] + [_vp] * 12 + [_vp, _i64, _vp], _i),
    "d3ga_skeleton_check": ([_sk] + [ctypes.c_int32] * 3, _i),
    "d3ga_skeleton_fwd": ([_sk] + [ctypes.c_int32] * 3 + [_vp, _vp, ctypes.c_int32, _vp, _vp, _f, ctypes.c_int32] + [_vp] * 4 + [_vp], _i),
    "d3ga_skeleton_bwd": ([_sk] + [ctypes.c_int32] * 4 + [_vp, _f, ctypes.c_int32] + [_vp] * 8 + [_vp], _i),
    "d3ga_skeleton_mats_fwd": ([ctypes.c_int32, ctypes.c_int32, _vp, _vp, _vp, _vp], _i),
    "d3ga_skeleton_mats_bwd": ([ctypes.c_int32, ctypes.c_int32, _vp, _vp, _vp, _vp, _vp], _i),
    "d3ga_vgg_panel_bytes": ([ctypes.c_int32, ctypes.c_int32], _i64),
    "d3ga_vgg_pack_weights": ([ctypes.c_int32, ctypes.c_int32, _vp, ctypes.c_int32, _vp, _vp], _i),
    "d3ga_vgg_conv3x3": ([ctypes.c_int32] * 4 + [_vp] * 4 + [ctypes.c_int32] * 2 + [_vp, _vp], _i),
    "d3ga_vgg_maxpool2_fwd": ([ctypes.c_int32] * 3 + [_vp, _vp, _vp], _i),
    "d3ga_vgg_maxpool2_bwd": ([ctypes.c_int32] * 3 + [_vp, _vp, _vp, _vp], _i),
    "d3ga_vgg_box_down2_fwd": ([ctypes.c_int32] * 4 + [_vp, _vp, _vp], _i),
    "d3ga_vgg_box_down2_bwd": ([ctypes.c_int32] * 4 + [_vp, _vp, _vp], _i),
    "d3ga_vgg_scratch_bytes": ([ctypes.c_int32] * 4 + [ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(_i64)], _i),
    "d3ga_vgg_conv3x3_n": ([ctypes.c_int32] * 5 + [_vp] * 4 + [ctypes.c_int32] * 2 + [_vp, _vp], _i),
    "d3ga_vgg_maxpool2_fwd_n": ([ctypes.c_int32] * 4 + [_vp, _vp, _vp], _i),
    "d3ga_lpips_input": ([ctypes.c_int32] * 4 + [_vp, _vp, _vp], _i),
    "d3ga_lpips_tap": ([ctypes.c_int32] * 4 + [_vp] * 6 + [ctypes.c_int32, _vp], _i),
    "d3ga_lpips_scratch_bytes": ([ctypes.c_int32] * 3 + [ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(_i64)], _i),
    "d3ga_code_lookup_fwd": ([_vp, _vp] + [ctypes.c_int32] * 3 + [_f, _vp, _vp], _i),
    "d3ga_code_lookup_bwd": ([_vp, _vp] + [ctypes.c_int32] * 3 + [_vp, _vp], _i),
    "d3ga_table_mean_scratch_bytes": ([ctypes.c_int32] * 2 + [ctypes.POINTER(_i64)], _i),
    "d3ga_table_mean": ([_vp] + [ctypes.c_int32] * 2 + [_vp, _vp, _vp], _i),
    "d3ga_row_cache_select": ([ctypes.POINTER(RowPair), ctypes.c_int32, _vp, _vp, _vp, _vp], _i),
    "d3ga_row_cache_flush": ([ctypes.POINTER(RowPair), ctypes.c_int32, _vp, _vp, _vp], _i),
    "d3ga_scale_energy_fwd": ([_i64, _vp, _vp, ctypes.c_int32, _vp, _vp, _vp], _i),
    "d3ga_scale_energy_bwd": ([_i64, _vp, _vp, ctypes.c_int32, _vp, _vp, _vp], _i),
    "d3ga_objective_fwd": ([ctypes.POINTER(ObjectiveDesc), _vp, _vp, _vp], _i),
    "d3ga_objective_bwd": ([ctypes.POINTER(ObjectiveDesc), _vp, _vp, _i64, _vp], _i),
    "d3ga_pose_fit_scratch_bytes": ([ctypes.c_int32] * 2 + [ctypes.POINTER(_i64)], _i),
    "d3ga_pose_fit": ([_vp] + [ctypes.c_int32] * 2 + [_vp, _vp, _vp], _i),
    "d3ga_pose_clamp": ([_vp, _vp] + [ctypes.c_int32] * 4 + [_vp] * 4 + [ctypes.c_double, ctypes.c_int32, _vp, _vp, _vp], _i),
    "d3ga_frame_grid_check": ([ctypes.POINTER(GridDesc), _vp, ctypes.POINTER(ctypes.c_int32)], _i),
    "d3ga_frame_grid": ([ctypes.POINTER(GridDesc), _vp, ctypes.POINTER(ctypes.c_int32), _vp], _i),
    "d3ga_png_capacity": ([ctypes.c_int32] * 4 + [ctypes.POINTER(_i64)], _i64),
    "d3ga_png_check": ([ctypes.c_int32] * 3 + [_i64, ctypes.c_int32, ctypes.c_int32, _vp, _vp, _i64, _vp, _i64], _i),
    "d3ga_png_encode": ([ctypes.c_int32] * 3 + [_i64, ctypes.c_int32, ctypes.c_int32, _vp, _vp, _i64, _vp, _i64, _vp], _i),
    "d3ga_sample_prep_actorshq": ([ctypes.c_int32] * 5 + [_vp, _i64, _i64] * 3 + [ctypes.c_int32, ctypes.c_int32] + [_vp] * 4 +
                                  [ctypes.POINTER(ctypes.c_int32), _vp], _i),
    "d3ga_sample_prep_goliath": ([ctypes.c_int32] * 3 + [_vp, _i64, _i64, _i64, _vp, _i64, _i64] + [_vp] * 4 +
                                 [ctypes.POINTER(ctypes.c_int32), _vp], _i),
    "d3ga_label_vote": ([ctypes.c_int32] * 5 + [_vp, _vp, ctypes.c_int32, _i64, _i64, _vp, _vp, _vp, ctypes.c_int32, _vp], _i),
    "d3ga_label_majority": ([ctypes.c_int32] * 2 + [_vp, _vp, _vp], _i),
    "d3ga_label_median": ([ctypes.c_int32] + [_vp] * 3 + [_vp], _i),
    "d3ga_label_grow": ([ctypes.c_int32] * 2 + [_vp] * 4 + [_vp], _i),
    "d3ga_surface_sample_scratch_bytes": ([ctypes.c_int32, ctypes.POINTER(_i64)], _i),
    "d3ga_surface_sample": ([ctypes.c_int32] * 3 + [_vp] * 10 + [_i64, _vp, ctypes.c_int32, _vp], _i),
    "d3ga_vertex_normals_angle": ([ctypes.c_int32] * 2 + [_vp] * 4 + [ctypes.c_double] + [_vp] * 3 + [_vp], _i),
    "d3ga_loop_edge_keys": ([ctypes.c_int32] * 2 + [_vp] * 3 + [_vp], _i),
    "d3ga_loop_plan_scratch_bytes": ([ctypes.c_int32] * 2 + [ctypes.POINTER(_i64)], _i),
    "d3ga_loop_plan_build": ([ctypes.POINTER(LoopPlanTables)] + [_vp] * 5 + [_i64, _vp], _i),
    "d3ga_loop_subdivide": ([ctypes.POINTER(LoopPlanTables), ctypes.c_int32, _vp, _vp, ctypes.c_int32, _vp, _vp, _vp], _i),
    "d3ga_loop_faces": ([ctypes.POINTER(LoopPlanTables), _vp, _vp, _vp], _i),
    "d3ga_unpose": ([ctypes.c_int32] * 4 + [_vp] * 3 + [ctypes.c_int32] + [_vp] * 3 + [ctypes.c_int32, _vp, _vp, _vp], _i),
    "d3ga_cage_voxelize": ([ctypes.POINTER(VoxelGridDesc), ctypes.c_int32, ctypes.c_int32, _vp, _vp, _vp, _vp], _i),
    "d3ga_cage_fill": ([ctypes.POINTER(VoxelGridDesc), ctypes.c_int32, _vp, _vp, _vp, _vp], _i),
    "d3ga_cage_iso_scratch_bytes": ([ctypes.c_int32, ctypes.POINTER(_i64)], _i),
    "d3ga_cage_iso_count": ([ctypes.POINTER(VoxelGridDesc), _vp, _i64, _vp, _vp], _i),
    "d3ga_cage_iso_emit": ([ctypes.POINTER(VoxelGridDesc), ctypes.POINTER(CageIsoDesc), _vp, _i64, _vp], _i),
    "d3ga_cage_smooth": ([ctypes.POINTER(LoopPlanTables), ctypes.POINTER(CageSmoothDesc), _vp], _i),
    "d3ga_cage_components": ([ctypes.POINTER(LoopPlanTables), ctypes.c_int32, _vp, _vp, _vp], _i),
    # quadric decimation (decimate.hip)
    "d3ga_decimate_scratch_bytes": ([ctypes.c_int32, ctypes.POINTER(_i64)], _i),
    "d3ga_decimate_quadrics": ([ctypes.POINTER(LoopPlanTables), ctypes.POINTER(DecimateDesc), _vp], _i),
    "d3ga_decimate_candidates": ([ctypes.POINTER(LoopPlanTables), ctypes.POINTER(DecimateDesc), _vp], _i),
    "d3ga_decimate_collapse": ([ctypes.POINTER(LoopPlanTables), ctypes.POINTER(DecimateDesc), _vp], _i),
    "d3ga_decimate_faces": ([ctypes.POINTER(LoopPlanTables), ctypes.POINTER(DecimateDesc), _vp], _i),
}
EXPORTS = tuple(_SIGNATURES)


def lib():
    """The loaded library.  Raises D3GAError (never falls back) if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(_PATH):
            raise D3GAError(
                f"{_PATH} is missing: the HIP extension has not been built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (or python d3ga_amd/csrc/build.py). "
                "There is no CPU fallback for this path.")
        import torch  # noqa: F401  -- loads PyTorch-ROCm's HIP runtime first so the process holds one runtime
        L = ctypes.CDLL(_PATH)
        for name, (args, res) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = res
        if L.d3ga_version() != ABI_VERSION:
            raise D3GAError(f"libd3ga_hip.so version {L.d3ga_version()} does not match the Python layer ({ABI_VERSION})")
        info = (ctypes.c_int32 * (2 + 2 * len(KNOBS)))()
        L.d3ga_debug_defaults(info, len(info))
        if info[0] != 0 and os.environ.get("D3GA_ALLOW_ABLATION") != "1":
            raise D3GAError(f"{_PATH} is a timing-ablation build (D3GA_SCAN_ABL={info[0]}): its results are wrong by design. "
                            "Set D3GA_ALLOW_ABLATION=1 to load it for a timing run.")
        # The library reads no environment.  Tests and A/B runs set its debug knobs through THIS layer:
        # D3GA_KNOBS="merge_slots=256,tile_assign=1" (names: KNOBS) -> d3ga_debug_set at load.  Product runs leave it unset.
        spec = os.environ.get("D3GA_KNOBS", "")
        for item in filter(None, (x.strip() for x in spec.split(","))):
            name, _, val = item.partition("=")
            if name not in KNOBS:
                raise D3GAError(f"D3GA_KNOBS: unknown knob {name!r} (known: {', '.join(KNOBS)})")
            st = L.d3ga_debug_set(KNOBS.index(name), int(val))
            if st != 0:
                raise D3GAError(f"d3ga_debug_set({name}, {val}) failed with status {st}")
        _lib = L
    return _lib


def debug_defaults():
    """d3ga_debug_defaults() as a dict: scan_abl, diag, then knob name -> (compiled default, value in effect)."""
    info = (ctypes.c_int32 * (2 + 2 * len(KNOBS)))()
    check(lib().d3ga_debug_defaults(info, len(info)), "d3ga_debug_defaults")
    out = {"scan_abl": info[0], "diag": info[1]}
    for k, name in enumerate(KNOBS):
        out[name] = (info[2 + 2 * k], info[3 + 2 * k])
    return out


def debug_set(name, value=None):
    """Set a debug knob of the library (tests / A/B runs only); value None restores the compiled default."""
    check(lib().d3ga_debug_set(KNOBS.index(name), -2**31 if value is None else int(value)), "d3ga_debug_set")


def check(status, what):
    if status != 0:
        msg = lib().d3ga_status_string(status)
        raise D3GAError(f"{what} failed with status {status}: {msg.decode() if msg else '?'}")


def stream_handle():
    """Raw hipStream_t of torch's CURRENT stream on the current device (the stream every launch of this library goes to).
    `torch.cuda.current_stream()` costs ~40 us of host time per call on this build (an os.environ lookup inside
    `_get_device_index`); the raw accessor is a plain C call."""
    import torch
    raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
    if raw is not None:
        return ctypes.c_void_p(raw(torch.cuda.current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def f32c16(t):
    """float32, contiguous AND 16-byte aligned (the vectorised kernels load 16 bytes per lane).  `.contiguous()` keeps a
    contiguous VIEW with a storage offset as it is -- e.g. `imgs[1]` of an (N,3,H,W) batch with odd H*W, or `x[1:]` -- so such
    a tensor is copied here instead of being rejected by the C ABI (D3GA_E_CONFIG)."""
    if t is None:
        return None
    t = t.float().contiguous()
    if t.data_ptr() % 16:
        t = t.clone(memory_format=__import__("torch").contiguous_format)
    return t


def require_cuda(*tensors):
    """Every launch of this library goes to the CURRENT device's current stream (stream_handle): a tensor that lives on
    another GPU would be touched from the wrong device / an unordered stream, so that is refused here."""
    import torch
    cur = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise D3GAError("d3ga_amd ops run on the GPU only (tensor on %s); there is no CPU fallback" % t.device)
        if cur is None:
            cur = torch.cuda.current_device()
        if t.device.index != cur:
            raise D3GAError(f"tensor on {t.device} but the current device is cuda:{cur}: wrap the call in "
                            f"`with torch.cuda.device({t.device.index}):` (launches go to the current device's stream)")
