/*
 * d3ga.h -- C ABI of libd3ga_hip.so: the MI355X (gfx950) deform-and-rasterize hot path of D3GA.
 *
 * Every entry point is `extern "C"`, takes raw DEVICE pointers (unless marked host), element counts,
 * scalar settings and a HIP stream, and returns an int status:
 *      0  ok        <0  invalid argument (D3GA_E_*)        >0  a hipError_t from the runtime.
 * No entry point throws, allocates persistent device memory, or synchronises the stream (except
 * d3ga_compute_bary, an init-time call, and any call made with params.debug != 0, which synchronises and
 * checks after every kernel).  All scratch is caller-owned; the library keeps no mutable global state,
 * so it is re-entrant across devices and streams.  Tensors are dense, row-major, float32 unless stated;
 * index tensors are int32.
 *
 * Each entry point cites the interface of the reference (facebookresearch/D3GA, paths relative to its root)
 * that it replaces.  Rows refer to SURVEY.md sec. 8a.
 */
#ifndef D3GA_H
#define D3GA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: exactly the functions declared in this header are exported. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define D3GA_VERSION 112 /* (d3ga_raster_params::tile_cull was added under 112 behind per_view_geometry, 0 = the behaviour before it: factor_rows, per_view_appearance and per_view_background move up by four bytes, so callers must be rebuilt against this header; no entry point changed) (the d3ga_vgg_*, d3ga_bary_interp_* and the frame-state entry points d3ga_code_lookup_*, d3ga_table_mean*, d3ga_row_cache_*, and the objective's d3ga_scale_energy_*, d3ga_objective_* were added under 112: additions only, nothing existing changed) the cage deformation takes descriptor structs: d3ga_cage_deform_{fwd,bwd} replace the seven entry points of ABI 111, d3ga_lbs_cage_bwd takes the pose plan (d3ga_lbs_cage_bwd_pose is gone), no float-atomic vertex gradient; 111: per-view appearance and backgrounds for view-batched rendering (d3ga_raster_params::per_view_appearance, ::per_view_background: the ColorField configuration's batch of frames); 110 (round 6): view-batched rendering (d3ga_raster_params::n_views, d3ga_raster_scratch_bytes_views), d3ga_debug_set / D3GA_KNOB_* replace every environment knob, the opt-in list forwards of round 5 are gone (d3ga_raster_bin_sort_lists, d3ga_raster_params::block_lists), only the functions declared here are exported */

#define D3GA_OK 0
#define D3GA_E_NULL (-1)     /* required pointer is NULL */
#define D3GA_E_SIZE (-2)     /* negative / inconsistent size */
#define D3GA_E_CONFIG (-3)   /* unsupported combination (e.g. both shs and colors_precomp) */
#define D3GA_E_CAPACITY (-4) /* scratch buffer too small */

typedef void *d3ga_stream_t; /* hipStream_t */

int d3ga_version(void);
const char *d3ga_status_string(int status);
/* Debug knobs (host only, no device work).  The library reads NO environment variable; the one piece of mutable process state it
 * keeps is this table of integers, for tests and A/B timing runs (d3ga_amd/_lib.py applies D3GA_KNOBS="name=value,..." at load).
 * Product code never calls d3ga_debug_set; with every knob at its default the entry points are re-entrant across devices and streams.
 *   d3ga_debug_set(key, value): set knob `key` (D3GA_KNOB_*); value == D3GA_KNOB_DEFAULT restores the compiled default.
 *   d3ga_debug_defaults(out, n): out[0] = D3GA_SCAN_ABL the library was compiled with (0 = product; anything else is a TIMING
 *   ABLATION whose results are wrong by design -- the Python layer refuses such a library unless D3GA_ALLOW_ABLATION=1), out[1] = 1
 *   for a diagnostic (counter) build, then for knob k < D3GA_KNOB_COUNT: out[2 + 2k] = compiled default, out[3 + 2k] = value in
 *   effect; n = capacity of out in int32 (>= 2 + 2 * D3GA_KNOB_COUNT, else D3GA_E_SIZE). */
#define D3GA_KNOB_COMPOSITE_VARIANT 0 /* bit 5 (32) work-ordered dispatch of the compositing kernels, bit 7 (128) exact block culling; default 160 */
#define D3GA_KNOB_MERGE_SLOTS 1       /* slots of the compositing backward's per-tile merge cache: 256 | 512 (default) */
#define D3GA_KNOB_TILE_ASSIGN 2       /* block -> wavefront assignment of the compositing backward: 0 quadrants, 1 interleaved, 2 by list length (default); +8: no early exit */
#define D3GA_KNOB_BWD_SPLIT 3         /* compositing backward: -1 (default) the D3GA_CNT_HEAVY heaviest tiles get two workgroups, 0 none, n > 0 the n heaviest */
#define D3GA_KNOB_SORT_MERGE 4        /* -1 (default) by size: the 2049..4096 list class rides in the 8192-key sort launch when few such lists are expected; 0 never; 1 always */
#define D3GA_KNOB_SSIM_IMPL 5         /* 1 (default) the marching register-window SSIM kernels, 0 the LDS-tiled ones of round 3 */
#define D3GA_KNOB_WGRAD_WS 6          /* 1 (default) the wavefront-specialised weight-gradient kernel for two wide operands and for a narrow dPre, 0 the barrier-phased one, 2 wavefront-specialised for every shape */
#define D3GA_KNOB_CHAIN_ABL 7         /* 0 (default); != 0: TIMING ablations of the fused field-network kernel (wrong results) */
#define D3GA_KNOB_CHAIN_GRID 8        /* 0 (default) = 2048 / wavefronts per workgroup; > 0: workgroups of the fused field-network kernel */
#define D3GA_KNOB_COUNT 9
#define D3GA_KNOB_DEFAULT (-2147483647 - 1)
int d3ga_debug_set(int32_t key, int32_t value);
int d3ga_debug_defaults(int32_t *out, int32_t n);

/* ---------------------------------------------------------------------------------------------------------
 * D0  Linear blend skinning of cage vertices (K-sparse weights).
 * Replaces: lib/smplman.py:155-171 Smplman.deform  (T = W.A ; v' = T[v+delta;1] ; v'.Rh^T + Th) and
 *           lbsmodel/body_model.py:208-234 LinearBlendSkinning.skinning (8-sparse form).
 *   tmpl (V,3), delta (V,3)|NULL, joint_mats (J,4,4), skin_idx (V,K) int32, skin_w (V,K),
 *   Rh (3,3)|NULL, Th (3)|NULL  ->  out (V,3).
 * bwd: grad_out (V,3) -> grad_delta (V,3)  (= gradient w.r.t. the template offset / deformation_field output).
 * bwd with pose != NULL: the same plus the pose gradients (the body pose reaches the cage through joint_mats, Rh and Th).  With
 *   p~ = [tmpl + delta; 1], o = (sum_k w_k A[idx_k]) p~, g = grad_out and g' = Rh^T g:
 *     g_joint_mats[j][0:3][0:4] = sum over the (v,k) with idx = j of w_vk g'_v p~_v^T, row 3 = 0 (the forward never reads it);
 *     g_Rh = sum_v g_v o_v^T (3,3);  g_Th = sum_v g_v (3).
 *   A joint listed twice in a row counts twice; a joint with no entry gets exact zeros.  The sums follow a static by-joint
 *   plan (struct d3ga_lbs_pose_grad, built once per binding: d3ga_amd/cage_deform.py lbs_pose_plan) in a fixed order, with no
 *   float atomics: repeated calls are bit-identical.  One launch after the per-vertex one (which runs unchanged, so grad_delta
 *   is bit-identical with and without pose): a by-joint reduction whose last workgroup forms the totals.  No host
 *   synchronisation, capturable.  pose needs V > 0 (else D3GA_E_SIZE).
 * ------------------------------------------------------------------------------------------------------- */
/* The by-joint plan and the outputs of the pose backward.  entries (n_entries = V*K): the flat indices v*K + k of skin_idx
 * sorted by joint (stable); chunk_range (n_chunks, 2; 8-byte aligned): [begin, end) of each chunk of entries, at most 256
 * entries, never straddling a joint; chunk_ptr (J + 1): the first chunk of each joint.  Every skin_idx must lie in [0, J).
 * tmpl (V,3), delta (V,3) | NULL: the forward's inputs.  counter: one uint32 of the plan, zero when the plan is built and left
 * zero by every call (its last workgroup re-arms it), so calls that share a plan run one after another (one stream).
 * scratch: d3ga_lbs_pose_scratch_bytes (4-byte aligned; no initialisation needed).  g_joint_mats (J,4,4), g_Rh (9), g_Th (3):
 * written (never accumulated), all three required. */
typedef struct d3ga_lbs_pose_grad {
    int32_t J;
    int32_t n_chunks;
    int64_t n_entries;
    const float *tmpl;
    const float *delta;
    const int32_t *chunk_ptr;
    const int32_t *chunk_range;
    const int32_t *entries;
    uint32_t *counter;
    void *scratch;
    float *g_joint_mats;
    float *g_Rh;
    float *g_Th;
} d3ga_lbs_pose_grad;
/* bytes of scratch for V vertices and n_chunks chunks; fused = 1 for d3ga_cage_deform_bwd, 0 for d3ga_lbs_cage_bwd */
int d3ga_lbs_pose_scratch_bytes(int V, int32_t n_chunks, int32_t fused, int64_t *bytes);
int d3ga_lbs_cage_fwd(int V, int K, const float *tmpl, const float *delta, const float *joint_mats,
                      const int32_t *skin_idx, const float *skin_w, const float *Rh, const float *Th, float *out,
                      d3ga_stream_t stream);
int d3ga_lbs_cage_bwd(int V, int K, const float *joint_mats, const int32_t *skin_idx, const float *skin_w,
                      const float *Rh, const float *grad_out, float *grad_delta, const d3ga_lbs_pose_grad *pose,
                      d3ga_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * D1-D5  Fused tetrahedral-cage deformation.
 * Replaces: models/cage_net.py:218-230 (tetpoints[tetra_faces], compute_def_grad, J S J^T, strip_symmetric,
 *           einsum bary means) with lib/cage.py:339-342 and utils/general_utils.py:24-35,58-90.
 * fwd: (inputs) -> means3D (P,3), cov6 (P,6) in order xx,xy,xz,yy,yz,zz.
 * bwd: (inputs, grads, route | NULL, skin | NULL, pose | NULL).  The vertex gradient is a scatter-add over 4 corners x P
 *   Gaussians; the route says how it is summed.  Both routes add in a fixed order without float atomics: repeated calls are
 *   bit-identical.  There is no other way to it (the float-atomic fallback of ABI <= 111 is gone).  Without skin and with
 *   P > 0, g_tetpoints and route come together: g_tetpoints without a route, and a route without g_tetpoints, both return
 *   D3GA_E_NULL; with neither, the per-Gaussian gradients alone are computed.
 *   P == 0 without skin: g_tetpoints | NULL is zeroed, the route is not looked at, nothing is launched.  P == 0 with skin: no
 *   Gaussian kernel runs, but the gather does, over the route's vert_start (V+1 zeros: all-empty lists; required, else
 *   D3GA_E_NULL), and writes g_delta (from g_tetpoints_extra alone) and the vertex gradient as described at
 *   d3ga_cage_deform_skin.  n_segments must be 0 then (else D3GA_E_SIZE) and no other pointer of the route is read: vert_items,
 *   records and the block plan may be NULL, as the pointers of empty tensors are.
 *   Status: a NULL inputs / grads struct or a missing required pointer D3GA_E_NULL; a negative size, K <= 0 or pose with
 *   V == 0 D3GA_E_SIZE; an unknown flag or route kind, a misaligned item_pos, skin without the merge route or pose without
 *   skin D3GA_E_CONFIG.
 * ------------------------------------------------------------------------------------------------------- */
#define D3GA_DEFORM_LOG_SCALES 1 /* `scales` holds log-scales: exp() applied inside, g_scales is d/d(log-scale) */
#define D3GA_DEFORM_GRAD_PER_TET 2 /* `canon_grad` is (T,3,3), one matrix per tetrahedron, read through tetra_id (the reference
                                    * stores the same matrices gathered per Gaussian, lib/cage.py:329: 36 B x P per pass) */
/* Inputs.  P Gaussians, V cage vertices (read by the backward only), flags = D3GA_DEFORM_*.  tetpoints (V,3) posed cage
 * vertices; tetras (T,4) int32; tetra_id (P) int32; barys (P,4); canon_grad (P,3,3) | (T,3,3) = inv(Dm) (lib/cage.py:329);
 * scales (P,3) activated, or log-scales under D3GA_DEFORM_LOG_SCALES; rots (P,4) wxyz (normalised inside); delta_barys (P,4)
 * | NULL is added to barys (models/cage_net.py:213-214 fused; g_barys is then the gradient of both). */
typedef struct d3ga_cage_deform_in {
    int32_t P, V, flags, reserved;
    const float *tetpoints;
    const int32_t *tetras, *tetra_id;
    const float *barys, *canon_grad, *scales, *rots, *delta_barys;
} d3ga_cage_deform_in;
/* Gradients.  In: g_means (P,3), g_cov6 (P,6).  Out, each | NULL (skipped): g_tetpoints (V,3), g_barys (P,4), g_scales (P,3),
 * g_rots (P,4). */
typedef struct d3ga_cage_deform_grads {
    const float *g_means, *g_cov6;
    float *g_tetpoints, *g_barys, *g_scales, *g_rots;
} d3ga_cage_deform_grads;
/* Vertex-gradient route over the static binding (tetras, tetra_id); built once (d3ga_amd/cage_deform.py).
 * D3GA_DEFORM_ROUTE_CORNERS (vertex_adjacency): the kernel writes its corner gradients to records (P,4,3); vert_start (V+1) /
 *   vert_items (4P) list, per vertex, the items 4*gaussian + corner incident to it; one wavefront per vertex adds them.
 *   item_pos, seg_ptr, seg_begin, n_segments are not read.
 * D3GA_DEFORM_ROUTE_MERGE (merge_plan; round 4): the corner gradients are merged per WORKGROUP before they leave the CU.  For
 *   every block of 256 consecutive Gaussians, item_pos (P,4 u16; 8-byte aligned) = position of item 4 i + corner among the
 *   block's items sorted by cage vertex, seg_ptr (blocks + 1) / seg_begin (n_segments, u16) = the runs of equal vertex; the
 *   kernel sums every run in LDS and writes one partial per run to records (n_segments,3); vert_start (V+1) / vert_items
 *   (n_segments) list each vertex's partials, which the vertex gather adds.  With spatially coherent numbering
 *   (tetra.spatial_order) a block has a few hundred runs instead of 1024 items.
 *   A binding without Gaussians (P == 0, with the skinning tail) has n_segments == 0 and needs vert_start (V+1 zeros) only:
 *   vert_items, records, item_pos, seg_ptr and seg_begin may be NULL. */
#define D3GA_DEFORM_ROUTE_CORNERS 1
#define D3GA_DEFORM_ROUTE_MERGE 2
typedef struct d3ga_cage_deform_route {
    int32_t kind, n_segments;
    const uint16_t *item_pos, *seg_begin;
    const int32_t *seg_ptr, *vert_start, *vert_items;
    float *records;
} d3ga_cage_deform_route;
/* Skinning tail (round 5; merge route only): the posed cage vertices came from d3ga_lbs_cage_fwd (lib/smplman.py:155-171 feeding
 * models/cage_net.py:218), so the LBS backward of D0 runs in the vertex-gather launch, on the gathered vertex gradient while
 * it sits in registers: g_delta (V,3; required) = (sum_k w_k A_k[:3,:3])^T Rh^T dL/d(tetpoint).  K, joint_mats, skin_idx, skin_w,
 * Rh | NULL: as d3ga_lbs_cage_bwd.  g_tetpoints_extra (V,3) | NULL: a gradient that reaches the posed vertices by another route
 * (the FEM regulariser), added before the skinning.  g_tetpoints is optional here and V == 0 launches nothing.
 * With pose (V > 0) one by-joint reduction launch follows, as in d3ga_lbs_cage_bwd, with g = the gathered vertex gradient
 * plus g_tetpoints_extra, kept in g_tetpoints or, when that is NULL, in pose->scratch; every other output is bit-identical
 * with and without pose. */
typedef struct d3ga_cage_deform_skin {
    int32_t K, reserved;
    const float *joint_mats;
    const int32_t *skin_idx;
    const float *skin_w, *Rh, *g_tetpoints_extra;
    float *g_delta;
} d3ga_cage_deform_skin;
int d3ga_cage_deform_fwd(const d3ga_cage_deform_in *in, float *means3D, float *cov6, d3ga_stream_t stream);
int d3ga_cage_deform_bwd(const d3ga_cage_deform_in *in, const d3ga_cage_deform_grads *grads, const d3ga_cage_deform_route *route,
                         const d3ga_cage_deform_skin *skin, const d3ga_lbs_pose_grad *pose, d3ga_stream_t stream);
/* The tails of d3ga_cage_deform_bwd alone -- the vertex gather the route asks for, with the skinning backward in it when `skin`
 * is given, and the by-joint reduction of `pose` -- on records that are ALREADY filled: by d3ga_raster_preprocess_bwd_deform (and
 * the two chained backwards built on it), which runs the per-Gaussian part of this backward inside the rasterizer's.  Same
 * arguments and status codes as d3ga_cage_deform_bwd; in->P, in->V and the route, skin and pose are read, grads->g_tetpoints is
 * written as there, and no other pointer of `in` / `grads` is looked at. */
int d3ga_cage_deform_bwd_tail(const d3ga_cage_deform_in *in, const d3ga_cage_deform_grads *grads, const d3ga_cage_deform_route *route,
                              const d3ga_cage_deform_skin *skin, const d3ga_lbs_pose_grad *pose, d3ga_stream_t stream);

/* D6  FEM regulariser (lib/cage.py:349-361): per-tet energy 0.5(det F-1)^2 + 0.5(|F|_F^2-3), F = Ds Dn^-1.
 *   fwd: energy (T).  bwd: g_energy (T) -> g_tetpoints (V,3) [zeroed by the call]. */
int d3ga_fem_energy_fwd(int T, const float *tetpoints, const int32_t *tetras, const float *Dn_inv, float *energy,
                        d3ga_stream_t stream);
int d3ga_fem_energy_bwd(int T, int V, const float *tetpoints, const int32_t *tetras, const float *Dn_inv,
                        const float *g_energy, float *g_tetpoints, d3ga_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * D2b  Barycentric attributes over a static binding (added without an ABI number change: new entry points only).
 * Replaces: the gather + einsum("ikj,ik->ij", attr[cells][cell_id], barys) wherever it is applied to data other than the posed
 *           cage: models/cage_net.py:236-241 (the ambient-occlusion value through cage_to_body_vertex, tetra_faces, tetra_id
 *           into `shadow`), models/cage_net.py:270 (canonical_means3D) and models/mesh_net.py:193,226 (the means of the mesh
 *           primitive: barycentric points on body-mesh triangles).
 *   attr (V,C); rows (P,K) int32: corner k of Gaussian i reads row rows[i,k] of attr -- the binding as ONE table, built once
 *   (d3ga_amd/bary_interp.py BaryBinding: tetras[tetra_id], vertex_map[tetras[tetra_id]] or the mesh's (P,3) face ids);
 *   barys (P,K); delta_barys (P,K) | NULL is added to barys (models/cage_net.py:213 fused)  ->  out (P,C).
 *   Domain: K in {3, 4}, 1 <= C <= 8, P >= 0, V >= 0, K P <= INT32_MAX.  With K == 4 rows, barys, delta_barys and g_barys are
 *   read / written 16 bytes per Gaussian and must be 16-byte aligned.  rows are NOT range-checked (the binding validates them).
 * fwd: w_k = barys[i,k] + delta_barys[i,k] (one rounding; barys[i,k] itself without delta_barys);
 *   out[i,c] = w_0 a_0, then fmaf(w_k, a_k, .) for k = 1 .. K-1 in that order, a_k = attr[rows[i,k], c].
 * bwd: g_out (P,C) -> g_barys (P,K) | NULL and g_attr (V,C) | NULL (each skipped when NULL).
 *   g_barys[i,k] = a_0 g_0, then fmaf(a_c, g_c, .) for c = 1 .. C-1, a_c = attr[rows[i,k], c], g_c = g_out[i,c]; it is the
 *   gradient of barys and of delta_barys.
 *   g_attr[v,c] = sum over the items of v of w g_out, a GATHER over the CSR lists vert_start (V+1) / vert_items (K P; item
 *   K i + k, built over the FINAL row ids), 16 lanes per row v: lane l adds the items at list positions l, l + 16, l + 32, ...
 *   of v's list in that order (s = 0; s = fmaf(w, g_out[i,c], s)), then the 16 lane sums are added by a butterfly over lane
 *   distance 1, 2, 4, 8.  No float atomics, the order depends on the lists alone: repeated calls are bit-identical.  Every row
 *   of g_attr is written (an empty list gives 0); the caller never zeroes it.
 *   P == 0: the forward launches nothing; the backward zeroes g_attr | NULL and reads no other pointer.
 *   Status, before any HIP call: a negative size, K not in {3, 4}, C outside 1..8 or K P > INT32_MAX D3GA_E_SIZE; with P > 0 a
 *   NULL attr, rows, barys, out / g_out, or g_attr without vert_start / vert_items D3GA_E_NULL; a misaligned pointer with
 *   K == 4 D3GA_E_CONFIG.  No host synchronisation, capturable.
 * ------------------------------------------------------------------------------------------------------- */
int d3ga_bary_interp_fwd(int32_t P, int32_t K, int32_t C, const float *attr, const int32_t *rows, const float *barys,
                         const float *delta_barys, float *out, d3ga_stream_t stream);
int d3ga_bary_interp_bwd(int32_t P, int32_t V, int32_t K, int32_t C, const float *attr, const int32_t *rows, const float *barys,
                         const float *delta_barys, const float *g_out, const int32_t *vert_start, const int32_t *vert_items,
                         float *g_attr, float *g_barys, d3ga_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * B1  SMPL / SMPL-X body model (added without an ABI number change: new entry points only, no existing layout moves).
 * Replaces the un-vendored `tetra_sampler.body_model.SMPLlayer` as built at
 * lib/smplman.py:68-74 and called at lib/smplman.py:175 (`geom, T, A, bs = lbs_module(poses=, shapes=, Rh=, Th=,
 * expression=)`).  The model is a set of device tensors prepared once on the host (d3ga_amd/body_model.py):
 *   NS = n_shape + n_expr blend coefficients [beta; psi], NR = NS + 9 (J - 1) rows of blend directions.
 *   dirs (NR, ld): rows 0..NS the shape / expression directions, rows NS + 9 (j - 1) + 3 a + c the pose direction of
 *       (R_j - I)[a][c], each row the 3V offsets x0 y0 z0 x1 ..., zero beyond 3V; ld a multiple of D3GA_BODY_LD_ALIGN.
 *   skin weights twice: CSR by vertex (w_ptr (V+1), w_joint, w_val) and by joint (wt_ptr (J+1), wt_vert ascending,
 *       wt_val), every nonzero of the dense (V,J) matrix.
 *   J0 (J,3) = J_regressor v_template, Jdirs (NS,J,3) = J_regressor . shape / expression directions.
 *   parents (J), parents[0] = -1; the kinematic tree by level (level_ptr (n_levels + 1), level_joint (J): a joint's parent sits
 *       in an earlier level) and by children (child_ptr (J+1), child_joint (J-1)).
 *   hand_comps (2, n_hand_pca, 45) left then right, hand_mean (2,45): the compact SMPL-X pose layout only.
 * 2 <= J <= D3GA_BODY_MAX_JOINTS, 0 <= n_hand_pca <= 45 (else D3GA_E_SIZE).
 * Pose layouts (pose_width): 3J axis-angle rows in joint order, or for n_hand_pca > 0 and J = 55 the compact
 *   [body 66 | left-hand PCA n | right-hand PCA n | jaw, left eye, right eye 9], hands = PCA . comps + mean.  A width of
 *   3J is always the full layout, also when n_hand_pca = 45 makes the compact width 3J as well.
 * R_j = Rodrigues(theta_j) with t = |theta_j + 1e-8|; forward kinematics G_j = G_parent [R_j | J_j - J_parent];
 *   A_j = [RG_j | tG_j - RG_j J_j] (not including Rh, Th); bs = dirs^T [beta; psi; pf] (= v_posed - v_template);
 *   T_v = sum_j w_vj A_j; verts = R(Rh) T_v [v_template + bs; 1] + Th.
 * fwd: poses (B, pose_width), shapes (B, n_shape), expr (B, n_expr) | NULL (zeros), Rh (B,3) | NULL, Th (B,3) | NULL
 *   -> verts (B,V,3), T (B,V,4,4), A (B,J,4,4), bs (B,V,3), saved (B, D3GA_BODY_SAVED_FLOATS(J)): what the backward reads.
 * bwd: saved, T and bs of the forward, upstream gradients g_verts (B,V,3), g_T (B,V,4,4), g_A (B,J,4,4), g_bs (B,V,3), each
 *   NULL = zero -> g_poses (B, pose_width), g_shapes (B, n_shape), g_expr (B, n_expr), g_Rh (B,3), g_Th (B,3), each NULL =
 *   not written.  The bottom rows of T and A are constants: their gradients are ignored.  Every reduction goes through
 *   partial slabs summed in a fixed order (no atomics): two calls give bitwise-equal gradients.
 * scratch: caller-owned device memory of at least d3ga_body_model_scratch_bytes (host query) for the pass; not kept
 *   between calls.  No host synchronisation: the calls are capturable in a graph.
 * ------------------------------------------------------------------------------------------------------- */
#define D3GA_BODY_MAX_JOINTS 64
#define D3GA_BODY_MAX_SHAPE 32          /* n_shape + n_expr */
#define D3GA_BODY_LD_ALIGN 2048         /* floats */
#define D3GA_BODY_SAVED_FLOATS(J) (27 * (J) + 16)
typedef struct d3ga_body_model {
    int32_t V, J;               /* vertices, joints */
    int32_t n_shape, n_expr;    /* shape and expression coefficients */
    int32_t n_hand_pca;         /* hand PCA components of the compact SMPL-X pose layout, 0: none */
    int32_t ld;                 /* row stride of dirs in floats */
    int32_t n_levels;           /* levels of the kinematic tree */
    int32_t reserved;
    const float *v_template;    /* (V,3) */
    const float *dirs;          /* (NR, ld) */
    const int32_t *w_ptr, *w_joint;
    const float *w_val;
    const int32_t *wt_ptr, *wt_vert;
    const float *wt_val;
    const float *J0;            /* (J,3) */
    const float *Jdirs;         /* (NS,J,3) */
    const int32_t *parents, *level_ptr, *level_joint, *child_ptr, *child_joint;
    const float *hand_comps, *hand_mean;
} d3ga_body_model;
int d3ga_body_model_scratch_bytes(const d3ga_body_model *model, int32_t B, int64_t *fwd_bytes, int64_t *bwd_bytes);
int d3ga_body_model_fwd(const d3ga_body_model *model, int32_t B, int32_t pose_width, const float *poses, const float *shapes,
                        const float *expr, const float *Rh, const float *Th, float *verts, float *T, float *A, float *bs,
                        float *saved, void *scratch, int64_t scratch_bytes, d3ga_stream_t stream);
int d3ga_body_model_bwd(const d3ga_body_model *model, int32_t B, int32_t pose_width, const float *saved, const float *T,
                        const float *bs, const float *g_verts, const float *g_T, const float *g_A, const float *g_bs,
                        float *g_poses, float *g_shapes, float *g_expr, float *g_Rh, float *g_Th, void *scratch,
                        int64_t scratch_bytes, d3ga_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * R1-R6  Tile rasterizer.  Replaces the un-vendored package `diff_gaussian_rasterization`
 * (graphdeco-inria, branch dr_aa; /root/reference/.gitmodules:9-12) as called from renderer.py:79-141:
 * _C.rasterize_gaussians / _C.rasterize_gaussians_backward / _C.mark_visible.
 * ------------------------------------------------------------------------------------------------------- */
typedef struct d3ga_raster_params {
    int32_t P;           /* number of Gaussians */
    int32_t M;           /* SH coefficients per Gaussian in `shs` (stride), 0 if colors_precomp */
    int32_t sh_degree;   /* active degree 0..3 */
    int32_t W, H;        /* raster size (renderer.py:80-81) */
    float tanfovx, tanfovy; /* tan(FoV/2) (renderer.py:76-77).  tanfovx <= 0: CAMERA SLOT -- the kernels read both from device
                             * memory, campos[3] and campos[4] (campos is then 5 floats), so that a captured hipGraph can be
                             * replayed with another camera by rewriting one device buffer (d3ga_amd/cameras.py:CameraSlot).
                             * tanfovx == D3GA_CAMERA_SLOT_WINDOWED: WINDOWED camera slot, see below. */
    float scale_modifier;
    int32_t antialiasing; /* branch dr_aa [UPSTREAM-RECALL]: opacity x sqrt(max(2.5e-5, det(cov2D) / det(cov2D + 0.3 I))); D3GA passes 0 (renderer.py:92) */
    int32_t prefiltered;  /* accepted, ignored (renderer.py:90) */
    int32_t debug;        /* !=0: synchronise + check after every kernel (renderer.py:91 passes 0) */
    /* D8 (models/cage_net.py:139-159, 247-249: opacity = sigmoid(opacities)): 0 = `opacities` holds activated values
     * (upstream's contract); D3GA_OPACITY_SIGMOID = `opacities` holds LOGITS, the sigmoid is applied on load in
     * d3ga_raster_preprocess and dL_dopacity of d3ga_raster_preprocess_bwd is the gradient w.r.t. the logit. */
    int32_t opacity_activation;
    /* != 0: no backward will follow this forward (inference / no input requires a gradient): d3ga_raster_composite_fwd does
     * not write the per-4x4-block lists its backward walks, and the img buffer only needs d3ga_raster_img_bytes(..., 1) bytes
     * (2 x 4 B per pixel instead of + 128 B per duplicate of capacity).  Calling a backward entry point afterwards is an error
     * (D3GA_E_CONFIG). */
    int32_t forward_only;
    /* != 0: `acc` of the backward entry points is a buffer the CALLER keeps from call to call and guarantees to be all zero
     * on entry: d3ga_raster_backward / _l1 then skip their clear (a 64 B x P fill kernel per backward) and
     * d3ga_raster_preprocess_bwd zero-fills every record it consumed, so that the buffer is all zero again when it returns.
     * All backwards sharing one such buffer must be ordered on one stream. */
    int32_t acc_self_clearing;
    /* View-batched rendering (round 6; no counterpart upstream: the reference renders one camera per call, renderer.py:69).
     * 0 or 1: one camera (everything below reads as before).  k > 1: the SAME Gaussians seen from k cameras are rasterised in ONE
     * grid per stage -- the launches of a single avatar view fill a third of the chip, k views fill it.  Then
     *   viewmatrix / projmatrix are (k,16), campos (k,3) -- (k,5) for camera slots -- radii (k,P);
     *   geom / binning / img are sized by d3ga_raster_scratch_bytes_views and hold k x P records / k x tiles lists: view v's Gaussian
     *   i is record v P + i, its tile (tx, ty) is tile (v gy + ty) gx + tx; W, H, tanfov* are shared by the views, bg too unless per_view_background;
     *   out_color (k,3,H,W), out_invdepth (k,H,W), dL_dpix (k,3,H,W), the L1 target (k,3,H,W) and its loss = mean over all k images;
     *   d3ga_raster_composite_fwd2 / _bwd2: colors2 stays (P,3) (shared by the views), out_color2 / dL_dpix2 are (k,3,H,W);
     *   acc (k P, D3GA_ACC_STRIDE);  d3ga_raster_preprocess_bwd SUMS dL/dmeans3D, dL/dopacity, dL/dcov3D | (dL/dscales, dL/drots) and a
     *   precomputed colour's gradient over the views (see per_view_geometry / per_view_appearance for the per-view forms), writes dL_dmeans2D per view (k,P,3), and for SH colours needs dL_dcolors
     *   (k,P,3) = the per-view factors of the rank-1 SH gradient, from which dL_dsh (P,M,3), when given, is rebuilt in one pass
     *   (d3ga_sh_grad_from_views) -- one 12 M-byte row per Gaussian and BATCH instead of per view.
     * Every view's image and the summed gradients equal k single-view calls (same kernels, same arithmetic per view).
     * Not available batched (D3GA_E_CONFIG): d3ga_raster_recolor. */
    int32_t n_views;
    /* n_views > 1 only.  != 0: a batch of FRAMES, not only of cameras -- every view has its own geometry (the reference's batch
     * holds frames of different poses, train.py:218-221: the avatar is deformed per frame, its appearance parameters are shared):
     * means3D is (k,P,3) and cov3D_precomp (k,P,6) | scales (k,P,3) + rotations (k,P,4); their gradients are written PER VIEW,
     * (k,P,.), not summed; opacities and shs | colors_precomp stay (P,.) with gradients summed over the views unless
     * per_view_appearance is set. */
    int32_t per_view_geometry;
    /* (added under ABI 112, in front of the fields that only batches of views read)  0: a Gaussian is listed in every tile of the reference's rectangle, the square of ceil(3 sqrt(lambda_max)) around
     * its centre -- tile lists, the duplicate count D and the longest list are upstream's.  != 0: d3ga_raster_preprocess cuts that
     * rectangle down to the tiles the Gaussian's alpha >= 1/255 box reaches (the half extents the compositing forward culls with,
     * GeomBuf::xyh), so the entries that the forward would reject for every pixel of the tile are never scattered, sorted or read.
     * Images, radii and the visible count are unchanged bit for bit (a visible Gaussian keeps at least one tile); every tile's
     * list is a subsequence of the reference's, so D, the longest list, per-pixel n_contrib and the positions in the per-block
     * lists are those of the SHORTER lists.  Gradients agree up to the summation order of float atomics.  Read by
     * d3ga_raster_preprocess (and d3ga_raster_forward) only; the other stages follow the lists they are given. */
    int32_t tile_cull;
    /* n_views > 1, SH colours: rows between consecutive views' factors in the dL_dcolors handed to d3ga_raster_preprocess_bwd (0 = P).
     * The camera-sharded exchange keeps one extra row per view (the view's camera position) so that factors and positions travel in
     * ONE all-gather (d3ga_amd/dist.py): P + 1. */
    int32_t factor_rows;
    /* n_views > 1 only (ABI 111).  != 0: every view has its own colour and opacity -- the reference's ColorField configuration
     * (use_shs: false) evaluates both per frame from that camera's view direction and that frame's encodings
     * (models/cage_net.py:232-258): opacities is (k,P) -- view v's opacity of Gaussian i is opacities[v P + i], activated values or
     * logits under D3GA_OPACITY_SIGMOID alike -- and colors_precomp (k,P,3); d3ga_raster_preprocess_bwd writes dL_dopacity (k,P) and
     * dL_dcolors (k,P,3) PER VIEW, not summed (zeros for a view in which the Gaussian is culled).  Precomputed colours only: with
     * shs != NULL the preprocess entry points return D3GA_E_CONFIG (SH colours are view-dependent already).  Independent of
     * per_view_geometry: both together are the ColorField batch of frames.  With n_views <= 1 accepted and without effect (a
     * (1,P,.) tensor is a (P,.) one). */
    int32_t per_view_appearance;
    /* n_views > 1 only (ABI 111).  != 0: every view has its own background (the reference draws one per frame,
     * models/trainer.py:95-100): `bg` is (k,3) for d3ga_raster_composite_fwd / _fwd_l1 / _fwd2 / _bwd / _bwd_l1 / _bwd2 / _bwd_depth
     * and d3ga_raster_forward / _backward / _backward_l1.  bg2 (the silhouette background of _fwd2 / _bwd2, black in the reference)
     * stays (3,), shared by the views.  With n_views <= 1 accepted and without effect. */
    int32_t per_view_background;
} d3ga_raster_params;
#define D3GA_OPACITY_SIGMOID 1

/* Windowed camera slot (crop-window rasterization; lib/batch.py:186-198 of the reference renders every frame at a padded raster
 * size w x h that centres the principal point, renderer.py:36-47 then pastes the W x H window back out of it).
 * d3ga_raster_params::tanfovx == D3GA_CAMERA_SLOT_WINDOWED selects it.  campos then holds ONE ROW OF 9 FLOATS PER VIEW (device memory):
 *     centre (3) | tan(FoVx/2) | tan(FoVy/2) | w | h | ox | oy          (w, h, ox, oy: exact float integers)
 * (w, h) is the view's full raster size, (ox, oy) the window's offset in it (paste(): ox = 0 if left_w > right_w else w - W, oy
 * likewise); d3ga_raster_params::W, ::H are the WINDOW size, shared by the views of a batch, and every output image is W x H: the
 * pixel (x, y) of the full raster lands at ((y - oy) W + (x - ox)).  Every floating-point quantity stays in full-raster pixel
 * coordinates -- projection with (w, h), the tile rectangle clamped to the raster's tiles -- so images, radii and the per-Gaussian
 * records are bit-identical to a full-raster render followed by the paste; only tile indices and output addresses are shifted.
 * Tile grid of a window: aligned to the raster's 16-pixel grid, first tile (ox / 16, oy / 16), a fixed tiles_x(W) + 1 by
 * tiles_y(H) + 1 tiles per view (covers any offset; the tiles a view does not need stay empty); view v's tile (tx, ty) is tile
 * (v gyw + ty) gxw + tx.  A Gaussian whose rectangle misses the window is culled in that view's records (its radius stays the
 * full-raster one).  The binning buffer is then sized by d3ga_raster_scratch_bytes_window: behind the sections of
 * d3ga_raster_binning_layout it holds the window table (one int32 x4 row per view: ox, oy, w, h) that d3ga_raster_preprocess writes
 * from campos and the compositing kernels read.  Because the record lives in device memory, a captured graph is replayed with any
 * camera whose crop pastes to W x H.  Not available windowed (D3GA_E_CONFIG): d3ga_raster_recolor. */
#define D3GA_CAMERA_SLOT_WINDOWED (-1.0f)
#define D3GA_CAMERA_SLOT_WINDOWED_FLOATS 9

/* Byte sizes of the three caller-owned scratch buffers (the analogue of upstream's geomBuffer /
 * binningBuffer / imgBuffer).  d_capacity = capacity in (tile,Gaussian) duplicates of the binning lists.
 * sizes[0]=geom, sizes[1]=binning, sizes[2]=img.  Buffers must be 256-byte aligned. */
int d3ga_raster_scratch_bytes(int32_t P, int32_t W, int32_t H, int64_t d_capacity, int64_t sizes[3]);
/* Bytes of the img buffer alone; forward_only != 0: without the per-block lists (d3ga_raster_params.forward_only). */
int64_t d3ga_raster_img_bytes(int32_t W, int32_t H, int64_t d_capacity, int32_t forward_only);
/* The same for a batch of n_views cameras (d3ga_raster_params::n_views): d_capacity counts the duplicates of ALL views;
 * sizes[2] is the img buffer with (forward_only == 0) or without the per-block lists. */
int d3ga_raster_scratch_bytes_views(int32_t P, int32_t W, int32_t H, int32_t n_views, int64_t d_capacity, int32_t forward_only,
                                    int64_t sizes[3]);

/* The same for WINDOWED camera slots (see D3GA_CAMERA_SLOT_WINDOWED): W, H = the window size, the tile grid (tiles_x(W) + 1) x
 * (tiles_y(H) + 1) per view, the binning buffer with the window table behind its sections. */
int d3ga_raster_scratch_bytes_window(int32_t P, int32_t W, int32_t H, int32_t n_views, int64_t d_capacity, int32_t forward_only,
                                     int64_t sizes[3]);
/* offsets[0..5] as d3ga_raster_binning_layout for the window grid of a W x H window, offsets[6] the window table (n_views x int32 x4). */
int d3ga_raster_binning_layout_window(int32_t W, int32_t H, int32_t n_views, int64_t d_capacity, int64_t offsets[7]);

/* Byte offsets of the sections of the binning buffer, for inspection/tests:
 * offsets[0] counters (8 x u32), [1] tile_count (tiles x u32), [2] tile_start (tiles+1 x u32, exclusive prefix),
 * [3] tile_cursor (tiles x u32), [4] keys (d_capacity x u64: depth bits << 32 | index, grouped by tile),
 * [5] point_list (d_capacity x u32: Gaussian indices, each tile's segment ascending in (depth, index)). */
int d3ga_raster_binning_layout(int32_t W, int32_t H, int64_t d_capacity, int64_t offsets[6]);
/* Same for the image buffer: offsets[0] final_T (H*W f32), [1] n_contrib (H*W u32). */
int d3ga_raster_img_layout(int32_t W, int32_t H, int64_t offsets[2]);
/* ... and its per-block lists (absent from a forward_only buffer), for inspection/tests: offsets[0] blk_count (16 x tiles u32: the
 * length of the prefix of a block's list the backward walks = up to the last entry some pixel of the block blended),
 * [1] blk_list (16 x d_capacity {u32 1-based position in the tile's list, u32 Gaussian index}; block b of a tile whose list is
 * [begin, end) starts at element 16 begin + b (end - begin); b = 4 x quadrant + block within the quadrant). */
int d3ga_raster_img_layout_blocks(int32_t W, int32_t H, int64_t offsets[2]);

/* The binning buffer starts with 8 uint32 counters the host may read back after the forward:
 *   [0] D = duplicates required (sum of tiles touched)      [1] 1 if D > d_capacity (lists truncated: re-run)
 *   [2] longest tile list                                    [3] number of visible Gaussians
 *   [4] tiles with 4097..8192 entries   [5] tiles with > 8192 entries   [6] tiles with 2049..4096 entries   [7] reserved */
#define D3GA_CNT_D 0
#define D3GA_CNT_OVERFLOW 1
#define D3GA_CNT_MAXTILE 2
#define D3GA_CNT_VISIBLE 3
#define D3GA_CNT_BIG 4  /* tiles with 4097..8192 entries (72 KB-LDS sort kernel) */
#define D3GA_CNT_HUGE 5 /* tiles with more than 8192 entries (sorted in global memory) */
#define D3GA_CNT_MID 6  /* tiles with 2049..4096 entries (36 KB-LDS sort kernel) */
#define D3GA_CNT_HEAVY 7 /* (non-empty tiles + 9) / 10, or 0 beyond 4096 non-empty tiles: the head of the work order whose tiles get two workgroups each in the compositing backward */

/* R1 per-Gaussian stage + tile histogram.  Exactly one of (shs | colors_precomp) and of
 * ((scales,rotations) | cov3D_precomp) is non-NULL.  viewmatrix/projmatrix are the reference's transposed
 * 4x4 matrices (lib/cameras.py:68-74), campos (3): all DEVICE pointers.  radii (P) int32 is an output. */
int d3ga_raster_preprocess(const d3ga_raster_params *prm, const float *means3D, const float *shs,
                           const float *colors_precomp, const float *opacities, const float *scales,
                           const float *rotations, const float *cov3D_precomp, const float *viewmatrix,
                           const float *projmatrix, const float *campos, void *geom, void *binning,
                           int64_t d_capacity, int32_t *radii, d3ga_stream_t stream);
/* R2+R3 tile offsets (scan), scatter of (depth,index) keys, per-tile sort in LDS. */
int d3ga_raster_bin_sort(const d3ga_raster_params *prm, void *geom, void *binning, int64_t d_capacity,
                         d3ga_stream_t stream);
/* R4 front-to-back compositing.  bg (3) device; (k,3) for a batch of views with per_view_background.  out_color (3,H,W); out_invdepth (H,W)|NULL. */
int d3ga_raster_composite_fwd(const d3ga_raster_params *prm, const float *bg, const void *geom, const void *binning,
                              int64_t d_capacity, void *img, float *out_color, float *out_invdepth,
                              d3ga_stream_t stream);
/* R5 back-to-front compositing backward.  dL_dpix (3,H,W).  Accumulates (atomically) into acc (P, D3GA_ACC_STRIDE) float,
 * which the CALLER must have zeroed (d3ga_raster_backward does it itself): [0..2] dL/dmean2D (x,y in NDC-scaled units, z
 * unused), [3..5] dL/dconic (a, b/2, c), [6] dL/dopacity, [7..9] dL/dcolor, [10] dL/d(1/depth) (d3ga_raster_composite_bwd_depth), [11..15] pad.  One record = one 64-byte line:
 * the nine float atomics of a (tile, Gaussian) contribution then meet the memory side as ONE request (with the former
 * 48-byte stride half of the records straddled two lines: compositing backward 246 -> 185 us at C3). */
#define D3GA_ACC_STRIDE 16
int d3ga_raster_composite_bwd(const d3ga_raster_params *prm, const float *bg, const void *geom, const void *binning,
                              int64_t d_capacity, const void *img, const float *dL_dpix, float *acc,
                              d3ga_stream_t stream);
/* The same with the gradient of the inverse-depth image of branch dr_aa [UPSTREAM-RECALL]: dL_dinvdepth (H,W) | NULL, dL_dpix
 * (3,H,W) | NULL (at least one).  The inverse depth takes part as a fourth channel whose per-Gaussian "colour" is 1 / depth:
 * acc[10] receives dL/d(1/depth) = sum alpha T dL/dinvdepth, which d3ga_raster_preprocess_bwd chains into dL/dmeans3D
 * (always: the slot is zero otherwise).  A batch of views (n_views = k > 1, with or without per_view_background, full rasters or
 * windowed camera slots) takes dL_dinvdepth (k,H,W) next to dL_dpix (k,3,H,W): view v's plane is dL_dinvdepth + v H W, H x W the
 * window of a windowed slot (tests/test_gpu_composite_paths.py holds all six batched / windowed launches to the oracle). */
int d3ga_raster_composite_bwd_depth(const d3ga_raster_params *prm, const float *bg, const void *geom, const void *binning,
                                    int64_t d_capacity, const void *img, const float *dL_dpix, const float *dL_dinvdepth,
                                    float *acc, d3ga_stream_t stream);

/* Two images from one pass (an extension over upstream's rasterizer; the reference's training step renders every package
 * twice with the same geometry and opacities -- RGB, then constant silhouette colours on black, models/trainer.py:102-110):
 * colors2 (P,3) is blended with the same alphas into out_color2 over bg2; alpha, T, the tile lists and the early exit are
 * shared.  The backward adds the second image's dL/dpixel to dL/dalpha; NO gradient is produced for colors2 (constants).
 * geom / binning / img exactly as for the single-image calls. */
int d3ga_raster_composite_fwd2(const d3ga_raster_params *prm, const float *bg, const float *bg2, const void *geom,
                               const float *colors2, const void *binning, int64_t d_capacity, void *img, float *out_color,
                               float *out_color2, float *out_invdepth, d3ga_stream_t stream);
int d3ga_raster_composite_bwd2(const d3ga_raster_params *prm, const float *bg, const float *bg2, const void *geom,
                               const float *colors2, const void *binning, int64_t d_capacity, const void *img,
                               const float *dL_dpix, const float *dL_dpix2, float *acc, d3ga_stream_t stream);

/* L1 image loss fused into the backward (extension; the loss of SURVEY sec. 8d's frame, utils/loss_utils.py:29 l1_loss =
 * mean |image - target|): the compositing backward forms dL/dpixel = g_loss[0] / (3 W H) * sign(image - target) (+ dL_dpix
 * when given, else NULL) per pixel, instead of reading a (3,H,W) gradient image that a separate kernel had to write.
 * image = the forward's out_color; target (3,H,W), or target_cell = device cell holding its address (graph.TensorSlot);
 * g_loss = dL/dloss (device scalar).  d3ga_raster_backward_l1 = clear + this + d3ga_raster_preprocess_bwd. */
/* ... and its VALUE fused into the compositing forward (round 4): d3ga_raster_composite_fwd plus loss[0] = mean |out_color -
 * target|.  Every quadrant wavefront adds |colour - target| of its 64 pixels while the colours are still in registers and
 * leaves one partial (partials: at least 4 * ceil(W/16) * ceil(H/16) floats, scratch); a second one-workgroup kernel adds the
 * partials in index order (bit-reproducible).  Replaces the pass over the finished image (d3ga_l1_mean_fwd_ws). */
int d3ga_raster_composite_fwd_l1(const d3ga_raster_params *prm, const float *bg, const void *geom, const void *binning,
                                 int64_t d_capacity, void *img, float *out_color, float *out_invdepth, const float *target,
                                 const void *target_cell, float *loss, float *partials, d3ga_stream_t stream);
int d3ga_raster_composite_bwd_l1(const d3ga_raster_params *prm, const float *bg, const void *geom, const void *binning,
                                 int64_t d_capacity, const void *img, const float *image, const float *target,
                                 const void *target_cell, const float *g_loss, const float *dL_dpix, float *acc,
                                 d3ga_stream_t stream);
int d3ga_raster_backward_l1(const d3ga_raster_params *prm, const float *means3D, const float *shs, const float *scales,
                            const float *rotations, const float *cov3D_precomp, const float *viewmatrix,
                            const float *projmatrix, const float *campos, const float *bg, const void *geom,
                            const void *binning, int64_t d_capacity, const void *img, const float *image,
                            const float *target, const void *target_cell, const float *g_loss, const float *dL_dpix,
                            float *acc, float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dopacity, float *dL_dsh,
                            float *dL_dcolors, float *dL_dcov3D, float *dL_dscales, float *dL_drots, d3ga_stream_t stream);
/* Re-render of the SAME geometry (same means3D / covariance / opacities / camera / image size) with other colours: the
 * reference's training step renders an RGB and a silhouette pass from one package (models/trainer.py:102-110).
 * Copies the geometry records of geom_src (a d3ga_raster_preprocess result) to geom_dst and evaluates only the colour
 * (SH from this camera, or colors_precomp).  geom_dst is then used with the binning buffer of the first pass in
 * d3ga_raster_composite_fwd / _bwd / _preprocess_bwd; the binning buffer is only read by those. */
int d3ga_raster_recolor(const d3ga_raster_params *prm, const float *means3D, const float *shs,
                        const float *colors_precomp, const float *campos, const void *geom_src, void *geom_dst,
                        d3ga_stream_t stream);

/* R6 per-Gaussian backward.  Writes every element of the outputs (zeros for culled Gaussians):
 * dL_dmeans3D (P,3), dL_dmeans2D (P,3), dL_dopacity (P,1), and dL_dsh (P,M,3) | dL_dcolors (P,3),
 * dL_dcov3D (P,6) | (dL_dscales (P,3), dL_drots (P,4)).
 * SH path with dL_dsh == NULL and dL_dcolors != NULL: FACTORED SH gradient -- dL_dcolors receives the clamp-masked
 * dL/dcolour (the (P,3) factor of the rank-1 SH gradient, see d3ga_sh_grad_from_views); dL/dmeans3D is complete.
 * cov3D_precomp: the SAME tensor, unchanged, that the forward was given (or NULL with scales / rotations): since round 4 the
 * forward keeps no copy of a precomputed covariance in `geom` (24 B x P less written per frame), the backward reads it here;
 * cov3D_precomp == NULL without (scales, rotations) returns D3GA_E_NULL (ABI 101).
 * `geom` must be what d3ga_raster_preprocess / d3ga_raster_recolor of THIS library left for THIS prm (forward_only == 0): since
 * round 5 it carries, for SH colours with M <= 16 and 3 M a multiple of 4, d(colour)/d(view direction) of every Gaussian (36 B,
 * nine planes of P floats) from which the direction term of dL/dmeans3D is formed -- `shs` is then not read here at all
 * (it must still be non-NULL: it selects the SH path). */
int d3ga_raster_preprocess_bwd(const d3ga_raster_params *prm, const float *means3D, const float *shs,
                               const float *scales, const float *rotations, const float *cov3D_precomp,
                               const float *viewmatrix, const float *projmatrix, const float *campos,
                               const void *geom, const float *acc, float *dL_dmeans3D, float *dL_dmeans2D,
                               float *dL_dopacity, float *dL_dsh, float *dL_dcolors, float *dL_dcov3D,
                               float *dL_dscales, float *dL_drots, d3ga_stream_t stream);

/* Convenience: the whole forward / backward as one call (same stream, no synchronisation). */
int d3ga_raster_forward(const d3ga_raster_params *prm, const float *means3D, const float *shs,
                        const float *colors_precomp, const float *opacities, const float *scales,
                        const float *rotations, const float *cov3D_precomp, const float *viewmatrix,
                        const float *projmatrix, const float *campos, const float *bg, void *geom, void *binning,
                        void *img, int64_t d_capacity, float *out_color, int32_t *radii, float *out_invdepth,
                        d3ga_stream_t stream);
int d3ga_raster_backward(const d3ga_raster_params *prm, const float *means3D, const float *shs, const float *scales,
                         const float *rotations, const float *cov3D_precomp, const float *viewmatrix,
                         const float *projmatrix, const float *campos, const float *bg, const void *geom,
                         const void *binning, int64_t d_capacity, const void *img, const float *dL_dpix, float *acc,
                         float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dopacity, float *dL_dsh,
                         float *dL_dcolors, float *dL_dcov3D, float *dL_dscales, float *dL_drots,
                         d3ga_stream_t stream);

/* R6 with the per-Gaussian part of the cage deformation's backward as its TAIL, for a render whose means3D and cov3D_precomp are
 * the outputs of d3ga_cage_deform_fwd (models/cage_net.py:213-230 feeding the renderer): the thread of Gaussian i keeps dL/dmean
 * and dL/dcov in registers and runs the deform backward on them, instead of writing 36 B that d3ga_cage_deform_bwd reads back in
 * the next launch.  Arguments of the parent entry, then `deform` (the inputs d3ga_cage_deform_fwd was given; deform->P == prm->P),
 * `dgrads` (g_barys / g_scales / g_rots, each | NULL; g_means, g_cov6 and g_tetpoints are not read) and `route` | NULL, whose
 * records are filled as d3ga_cage_deform_bwd fills them.  The vertex gather and the skinning / pose tails are NOT launched:
 * d3ga_cage_deform_bwd_tail runs them on these records.  dL_dmeans3D and dL_dcov3D may BOTH be NULL here (not written; one without
 * the other is D3GA_E_CONFIG); dL/dSH, dL/dopacity and dL/dmean2D are the parent's bit for bit.  g_barys, g_scales, g_rots and the
 * records are those of the two calls up to the last bit of dL/dmean and dL/dcov (the compiler contracts the multiply-adds of values
 * that stay in registers differently) -- and bit for bit when the two arrays are requested, which are then written by the parent's
 * own code and taken from there.  One view on the full raster with a precomputed covariance only: n_views > 1, a windowed camera
 * slot, scales / rotations (or their gradients) return D3GA_E_CONFIG, as does every deform argument d3ga_cage_deform_bwd
 * refuses.  d3ga_raster_backward_deform / _l1_deform: the clear and the compositing backward of their parents, then this. */
int d3ga_raster_preprocess_bwd_deform(const d3ga_raster_params *prm, const float *means3D, const float *shs,
                                      const float *scales, const float *rotations, const float *cov3D_precomp,
                                      const float *viewmatrix, const float *projmatrix, const float *campos,
                                      const void *geom, const float *acc, float *dL_dmeans3D, float *dL_dmeans2D,
                                      float *dL_dopacity, float *dL_dsh, float *dL_dcolors, float *dL_dcov3D,
                                      float *dL_dscales, float *dL_drots, const d3ga_cage_deform_in *deform,
                                      const d3ga_cage_deform_grads *dgrads, const d3ga_cage_deform_route *route,
                                      d3ga_stream_t stream);
int d3ga_raster_backward_deform(const d3ga_raster_params *prm, const float *means3D, const float *shs, const float *scales,
                                const float *rotations, const float *cov3D_precomp, const float *viewmatrix,
                                const float *projmatrix, const float *campos, const float *bg, const void *geom,
                                const void *binning, int64_t d_capacity, const void *img, const float *dL_dpix, float *acc,
                                float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dopacity, float *dL_dsh,
                                float *dL_dcolors, float *dL_dcov3D, float *dL_dscales, float *dL_drots,
                                const d3ga_cage_deform_in *deform, const d3ga_cage_deform_grads *dgrads,
                                const d3ga_cage_deform_route *route, d3ga_stream_t stream);
int d3ga_raster_backward_l1_deform(const d3ga_raster_params *prm, const float *means3D, const float *shs, const float *scales,
                                   const float *rotations, const float *cov3D_precomp, const float *viewmatrix,
                                   const float *projmatrix, const float *campos, const float *bg, const void *geom,
                                   const void *binning, int64_t d_capacity, const void *img, const float *image,
                                   const float *target, const void *target_cell, const float *g_loss, const float *dL_dpix,
                                   float *acc, float *dL_dmeans3D, float *dL_dmeans2D, float *dL_dopacity, float *dL_dsh,
                                   float *dL_dcolors, float *dL_dcov3D, float *dL_dscales, float *dL_drots,
                                   const d3ga_cage_deform_in *deform, const d3ga_cage_deform_grads *dgrads,
                                   const d3ga_cage_deform_route *route, d3ga_stream_t stream);

/* View-sharded training (no reference counterpart: the reference trains on one GPU).  Per view v
 * the SH gradient is rank-1 per Gaussian: dL/dsh[i][k][c] = Y_k(normalize(means3D[i] - campos_v)) * g_v[i][c] with g_v the
 * factored output of d3ga_raster_preprocess_bwd.  Rebuilds  dL_dsh (P,M,3) = scale * sum_v Y(dir_v) (x) g_v  from the
 * gathered factors: g_views + v*g_stride -> (P,3) floats of view v, campos_views + v*campos_stride -> 3 floats
 * (strides in floats).  Coefficients k >= (sh_degree+1)^2 get 0. */
int d3ga_sh_grad_from_views(int32_t P, int32_t M, int32_t sh_degree, int32_t n_views, const float *means3D,
                            const float *g_views, int64_t g_stride, const float *campos_views, int64_t campos_stride,
                            float scale, float *dL_dsh, d3ga_stream_t stream);

/* _C.mark_visible: visible[i] = 1 if view-space z > 0.2 (uint8 output). */
int d3ga_raster_mark_visible(int32_t P, const float *means3D, const float *viewmatrix, uint8_t *visible,
                             d3ga_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Init-time point location.  Replaces tetra_sampler.compute_bary (lib/cage.py:325-327): for each point the
 * containing tetrahedron (point-in-tet per submodules/tetrahedralize/include/tet/tetrahedron.h:46-71) and its
 * barycentric weights (same header :77-101, order a,b,c,d); points outside every tet take the tet with the
 * largest minimum barycentric weight (weights may be negative) and active[i] = 0.
 *   points (P,3), tetra_corners (T,4,3) -> barys (P,4), tetra_id (P) int32, active (P) uint8.
 * ------------------------------------------------------------------------------------------------------- */
/* ---------------------------------------------------------------------------------------------------------
 * Loss tail.  Replaces utils/loss_utils.py:29  l1_loss = |network_output - gt|.mean().
 *   fwd: out[0] = mean |a - b| over n floats (out is zeroed by the call; float atomics across workgroups).
 *   bwd: grad_a = g[0] * sign(a - b) / n   (g: device scalar).   a, b, grad_a 16-byte aligned.
 * ------------------------------------------------------------------------------------------------------- */
int d3ga_l1_mean_fwd(int64_t n, const float *a, const float *b, float *out, d3ga_stream_t stream);
/* The same value in two stages: one partial sum per workgroup into `partials` (>= D3GA_LOSS_PARTIALS floats, contents
 * irrelevant), then one workgroup adds them in index order.  No zero fill, no atomics: the result is reproducible bit for
 * bit, and the call is ~2x faster at image sizes (the 512 same-address atomics of the form above serialise). */
#define D3GA_LOSS_PARTIALS 2048
int d3ga_l1_mean_fwd_ws(int64_t n, const float *a, const float *b, float *out, float *partials, d3ga_stream_t stream);
int d3ga_l1_mean_bwd(int64_t n, const float *a, const float *b, const float *g, float *grad_a, d3ga_stream_t stream);
/* The same two with `b` behind a device CELL: the kernels read its address from *b_cell (device memory) when they start.
 * A captured hipGraph is pointed at another resident target image by rewriting that 8-byte cell instead of copying the
 * image into a static buffer (d3ga_amd/graph.py: TensorSlot).  The tensor the cell names must be 16-byte aligned. */
int d3ga_l1_mean_fwd_ws_cell(int64_t n, const float *a, const float *const *b_cell, float *out, float *partials,
                             d3ga_stream_t stream);
int d3ga_l1_mean_bwd_cell(int64_t n, const float *a, const float *const *b_cell, const float *g, float *grad_a,
                          d3ga_stream_t stream);

/* 11x11 Gaussian-window SSIM, mean over all channels and pixels.  Replaces utils/loss_utils.py:46-86 (ssim / _ssim with
 * window_size = 11, sigma = 1.5, zero padding 5, size_average = True; called at train.py:192).
 *   fwd: img1, img2 (C,H,W) -> out[0] = mean ssim_map, written by the call (contents irrelevant before): every workgroup
 *        stores a partial sum in scratch the library owns and one workgroup adds them in index order -- the same bits on
 *        every call.  An eager launch uses the scratch slot of its (device, stream), a launch recorded into a graph keeps a
 *        slot for good: D3GA_E_CAPACITY beyond 64 streams or 192 recorded launches per process.
 *        Dm, Dq1, Dq12: optional (C,H,W) outputs
 *        (all three or none) holding d ssim_map / d(w*img1), d(w*img1^2), d(w*img1*img2) for the backward.
 *   bwd: grad_img1 (C,H,W) = g[0]/(C*H*W) * ( w*Dm + 2 img1 (w*Dq1) + img2 (w*Dq12) ),  g: device scalar dL/d(mean).
 * The gradient w.r.t. img2 is the same call with the two images swapped (SSIM is symmetric). */
int d3ga_ssim_fwd(int32_t C, int32_t H, int32_t W, const float *img1, const float *img2, float *out, float *Dm,
                  float *Dq1, float *Dq12, d3ga_stream_t stream);
int d3ga_ssim_bwd(int32_t C, int32_t H, int32_t W, const float *img1, const float *img2, const float *Dm,
                  const float *Dq1, const float *Dq12, const float *g, float *grad_img1, d3ga_stream_t stream);
/* The same two kernels with the L1 term of train.py:190-193 riding along (both losses read the same two images):
 * out_l1[0] = mean |img1 - img2| (NULL: skipped); g_l1: device scalar dL/d(l1) (NULL: no L1 term in the gradient). */
int d3ga_ssim_l1_fwd(int32_t C, int32_t H, int32_t W, const float *img1, const float *img2, float *out, float *Dm,
                     float *Dq1, float *Dq12, float *out_l1, d3ga_stream_t stream);
int d3ga_ssim_l1_bwd(int32_t C, int32_t H, int32_t W, const float *img1, const float *img2, const float *Dm,
                     const float *Dq1, const float *Dq12, const float *g, const float *g_l1, float *grad_img1,
                     d3ga_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Image tail of the Goliath configuration (configs/goliath_axe184.yml: use_blur), between render() and the losses.
 * Learnable blur, models/learnable_blur.py:34-44 (called at models/trainer.py:124-126):
 *     w = softmax(weights_raw[cam]);   out = w0 img + w1 B3(img) + w2 B7(img)
 * with Bk the separable k-tap Gaussian (sigma_k = 0.15 k + 0.35, taps exp(-(x / sigma_k)^2 / 2) normalised to sum 1)
 * over the image extended by k / 2 pixels of reflect padding (torchvision's gaussian_blur; -1 -> 1, H -> H - 2).
 *   img, out, grad_out, grad_img (C,H,W) f32; weights_raw, grad_weights_raw (n_cameras,3) f32; cam_idx: ONE int32 in
 *   DEVICE memory, read when the kernel starts (a captured step follows another camera by overwriting it) and clamped to
 *   [0, n_cameras).  H, W >= 4 (else D3GA_E_SIZE, nothing launched).
 *   fwd: one launch.
 *   bwd: grad_img = w0 g + w1 B3^T g + w2 B7^T g (B^T: the adjoint of blur-with-reflect-padding; NULL: skipped), and
 *        grad_weights_raw[cam][j] = w_j (s_j - sum_i w_i s_i) with s = (<g, img>, <B3^T g, img>, <B7^T g, img>), every
 *        other row 0: the whole tensor is written (NULL: skipped; img may then be NULL too).  The three sums go through
 *        `partials` (>= D3GA_BLUR_PARTIALS floats, contents irrelevant): one partial per workgroup, added in index order
 *        by a second launch -- no zero fill, no atomics, bit-reproducible.
 * ------------------------------------------------------------------------------------------------------- */
#define D3GA_BLUR_PARTIALS 6144
int d3ga_blur_mix_fwd(int32_t C, int32_t H, int32_t W, int32_t n_cameras, const float *img, const float *weights_raw,
                      const int32_t *cam_idx, float *out, d3ga_stream_t stream);
int d3ga_blur_mix_bwd(int32_t C, int32_t H, int32_t W, int32_t n_cameras, const float *img, const float *weights_raw,
                      const int32_t *cam_idx, const float *grad_out, float *grad_img, float *grad_weights_raw,
                      float *partials, d3ga_stream_t stream);
/* Target composition, train.py:182-188 (no gradient):  m = 1 - float(boundary_fg),
 *     gt_image = (image alpha + (1 - alpha) bg_c) m + (1 - m) bg_c,     gt_silhouette = silhouette alpha m
 * image, silhouette, gt_image, gt_silhouette (C,H,W) f32; alpha (H,W) f32; boundary_fg (H,W) uint8 / bool bytes, or f32
 * with boundary_is_float != 0; bg (C) f32 in device memory. */
int d3ga_compose_target(int32_t C, int32_t H, int32_t W, const float *image, const float *alpha, const float *silhouette,
                        const void *boundary_fg, int32_t boundary_is_float, const float *bg, float *gt_image,
                        float *gt_silhouette, d3ga_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Per-camera colour calibration of the Goliath configuration (configs/goliath_axe184.yml: use_color_calib),
 * lib/calibration.py:39-56 (called at models/garment_net.py:265-266):
 *     (w, b) = corrections[cam][:3], corrections[cam][3:];   out = rgb * w + b   per channel,
 * the product and the sum rounded separately (bit-equal to the float32 torch expression of lines 48-50); a view whose
 * camera is identity_idx is copied through unchanged (line 42-43; identity_idx < 0: no such camera).
 *   rgb, out, grad_out, grad_rgb: k views of n elements, f32, 16-byte aligned (else D3GA_E_CONFIG);
 *       planar == 0  (k,n,3) interleaved, the layout of pkg["rgb"] (line 50);
 *       planar == 1  (k,3,n) planes, the reference's image branch with n = H W (line 48).
 *   corrections, grad_corrections (n_cameras,6) f32; cam: k int32 in DEVICE memory, read when the kernels run and clamped
 *   to [0, n_cameras).  k >= 1, 3 k <= D3GA_CALIB_PARTIALS / 6, n >= 0, 3 k n <= INT32_MAX, n_cameras >= 1 (else
 *   D3GA_E_SIZE, nothing launched).  n == 0 is valid: no launch over elements, the element pointers may be NULL, and
 *   grad_corrections is still written (zeros).
 *   fwd: one launch.
 *   bwd: one pass over grad_out (and rgb, with grad_corrections != NULL): grad_rgb = g * w, or g for the identity camera
 *        (NULL: skipped), and per-workgroup partials of the six sums per view (sum g rgb and sum g per channel) in `partials`
 *        (>= D3GA_CALIB_PARTIALS floats, contents irrelevant).  A second, one-workgroup launch adds them in index order,
 *        multiplies by grad_scale (the reference's params.register_hook(... 1e-1) of lines 52-54: the parameter gradient only,
 *        in training mode only; pass 1 otherwise), adds the views that share a camera in view order and writes the WHOLE
 *        grad_corrections: zeros in every row whose camera is not in the batch and in the identity camera's row.  No atomics,
 *        no zero fill, bit-identical from run to run.  grad_corrections == NULL: skipped; rgb and partials may then be NULL.
 * ------------------------------------------------------------------------------------------------------- */
#define D3GA_CALIB_PARTIALS 12288
int d3ga_color_calib_fwd(int32_t k, int32_t n, int32_t planar, int32_t n_cameras, int32_t identity_idx, const float *rgb,
                         const float *corrections, const int32_t *cam, float *out, d3ga_stream_t stream);
int d3ga_color_calib_bwd(int32_t k, int32_t n, int32_t planar, int32_t n_cameras, int32_t identity_idx, float grad_scale,
                         const float *rgb, const float *corrections, const int32_t *cam, const float *grad_out,
                         float *grad_rgb, float *grad_corrections, float *partials, d3ga_stream_t stream);
/* Per-camera pixel bias (use_pixel_cal), models/color_calib.py:245-258 (added to the prediction at models/trainer.py:128-131):
 * up = F.interpolate(bias[cam], size=(H,W), mode='bilinear'), i.e. align_corners=False; per axis
 *     src = max(0, (dst + 0.5) n_in / n_out - 0.5),  i0 = floor(src),  i1 = min(i0 + 1, n_in - 1),  lambda = src - i0,
 * with src formed as the ratio of integers ((2 dst + 1) n_in - n_out) / (2 n_out): i0 exact, lambda one rounded quotient.
 *   bias, grad_bias (n_cameras,1,bh,bw) f32 (bh along H); cam: ONE int32 in device memory, clamped to [0, n_cameras).
 *   fwd: image != NULL: out (C,H,W) = image + up, up broadcast over the channels; image == NULL: out (1,H,W) = up (C is
 *        ignored beyond the size check).  One launch.
 *   bwd: grad_out (C,H,W) -> grad_bias[cam] = U_h^T (sum_c grad_out_c) U_w, gathered per low-resolution cell over the
 *        contiguous range of pixels that touch it (no atomics, bit-identical from run to run); the same launch writes zeros to
 *        every other camera's map.  dL/dimage is grad_out itself: there is no launch for it.
 *   All sizes >= 1, C H W and n_cameras bh bw <= INT32_MAX, H bh and W bw < 2^30 (else D3GA_E_SIZE, nothing launched). */
int d3ga_pixel_bias_fwd(int32_t C, int32_t H, int32_t W, int32_t n_cameras, int32_t bh, int32_t bw, const float *bias,
                        const int32_t *cam, const float *image, float *out, d3ga_stream_t stream);
int d3ga_pixel_bias_bwd(int32_t C, int32_t H, int32_t W, int32_t n_cameras, int32_t bh, int32_t bw, const int32_t *cam,
                        const float *grad_out, float *grad_bias, d3ga_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Frame preparation: the image path of Batcher.process (lib/batch.py:150-163, 180, 205-208, 236), one launch for B frames.
 * Per pixel, with s = int(seg_part) and fg = (s > 0) | (seg_fg > 0):
 *   orig        v / 255; with D3GA_FRAME_GAMMA linear2color_corr of it (utils/image_utils.py:92-113):
 *                   x = v / 255 * scale_c / 1.1,   clamp(sqrt(k clamp(x - black, 0, 2)) - 15/255, 0, 2)
 *               scale = (1.4, 1.1, 1.6), black = 3/255, k = float32((1 / (1 - black)) 0.95 in double); every operation
 *               rounded to float32 on its own, in this order, divide and square root correctly rounded;
 *   image       fg ? orig : bg, bg = 1 with D3GA_FRAME_BG_WHITE, else 0  (= orig fg + (1 - fg) resp. orig fg, fg being 0 or 1);
 *   silhouette  s == 0: bg in all three channels; 0 < s < n_labels: label_rgb[s]; every other s (negative ones too): other_rgb;
 *   alpha       1 iff at least 25 of the 49 pixels of the 7x7 window around the pixel are fg, pixels outside the image
 *               counting as 0 (kornia's median_blur of a 0 / 1 image: zero padding, the 25th smallest of 49); then with
 *               D3GA_FRAME_ERODE_MASK a 7x7 dilation and a 5x5 erosion, then with D3GA_FRAME_CLOSE_HOLES a 5x5 dilation and
 *               a 5x5 erosion (utils/image_utils.py:49-70), both over the in-image part of the window (kornia's geodesic
 *               border): dilation = some 1 in it, erosion = no 0 in it.
 *   image     (B,3,H,W) f32, or uint8 with D3GA_FRAME_IMAGE_U8;  seg_part (B,1,H,W) int32, or f32 with D3GA_FRAME_SEG_F32
 *   (truncated toward zero, as .int());  seg_fg (B,1,H,W) f32 or NULL (= zeros);  label_rgb (n_labels,3) f32, row 0 unused;
 *   other_rgb (3) f32;  image_out, orig_out, sil_out (B,3,H,W), alpha_out (B,1,H,W) f32: each may be NULL (skipped; without
 *   alpha_out no stage runs).  H and W may be smaller than any window.
 *   Status, nothing launched: B, H, W <= 0, n_labels < 1, B > 65535 or H W > INT32_MAX D3GA_E_SIZE; an unknown flag, or image /
 *   an output not 16-byte aligned D3GA_E_CONFIG; image, seg_part, label_rgb or other_rgb NULL, or every output NULL D3GA_E_NULL.
 *   No scratch, no atomics; capturable.
 * ------------------------------------------------------------------------------------------------------- */
#define D3GA_FRAME_GAMMA 1
#define D3GA_FRAME_BG_WHITE 2
#define D3GA_FRAME_ERODE_MASK 4
#define D3GA_FRAME_CLOSE_HOLES 8
#define D3GA_FRAME_IMAGE_U8 16
#define D3GA_FRAME_SEG_F32 32
#define D3GA_FRAME_ALL 63
int d3ga_frame_prep(int32_t B, int32_t H, int32_t W, int32_t flags, const void *image, const void *seg_part,
                    const float *seg_fg, const float *label_rgb, int32_t n_labels, const float *other_rgb, float *image_out,
                    float *orig_out, float *alpha_out, float *sil_out, d3ga_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Evaluation tail: what test.py does per frame between trainer.fit and the PNG writers (and train.py's progress report in
 * miniature), for B frames, in three launches.  No gradient.
 * d3ga_eval_frames, per pixel, every operation rounded to float32 on its own:
 *   a            alpha[0] (1 - float(boundary_fg))                                         test.py:140-141
 *   target       image a + (1 - a) bg,  bg = 1 with D3GA_EVAL_BG_WHITE, else 0             test.py:151
 *   ground_truth [image a, a], four channels                                               test.py:186-187
 *   heat         jet[bin],  e = sqrt(sum_c (target_c - pred_c)^2),  bin = min(int(min(e, 1) 256), 255), a NaN e: row 256;
 *                jet: matplotlib's 256-entry "jet" table times 255 truncated to uint8, divided by 255 in float32, plus the
 *                "bad" colour (0, 0, 0) as row 256                                          recorder/heatmap.py:16-34, 45-47
 *   partials     sum of (target_c - pred_c)^2 over the workgroup's pixels: d3ga_eval_partials(H, W) floats per (frame,
 *                channel), frame-major, stored plainly (contents irrelevant before the call)
 *   With D3GA_EVAL_COMPOSED `image` IS the target (compute_errors(target, fake) and compute_heatmap, heatmap.py:37-61): alpha
 *   and boundary_fg are not read and may be NULL; target_out and gt_out must be NULL then (D3GA_E_CONFIG).
 *   pred, image, target_out, heat_out (B,3,H,W) f32;  gt_out (B,4,H,W) f32;  alpha (B,1,H,W) f32, or (B,3,H,W) with
 *   D3GA_EVAL_ALPHA3 (channel 0 is read);  boundary_fg (B,1,H,W) uint8 / bool bytes, or f32 with D3GA_EVAL_BOUNDARY_F32.
 *   Every output may be NULL (skipped), not all of them.  With H W % 4 == 0 and every tensor 16-byte aligned (boundary_fg
 *   bytes: 4-byte) the planes are moved in 16-byte quads, otherwise pixel by pixel: same values either way.
 * d3ga_eval_ssim: the forward of the 11x11 Gaussian-window SSIM described at d3ga_ssim_fwd, for B frames of three channels, one
 *   plainly stored partial (the sum of ssim_map over a 16 x 16 tile) per tile: d3ga_eval_ssim_partials(H, W) floats per frame,
 *   frame-major, added in index order by d3ga_eval_finish.  pred, target (B,3,H,W) f32, element-aligned.
 * d3ga_eval_finish, one workgroup per frame: adds the frame's partials in index order (bit-reproducible),
 *   mse_c = sum_c / (H W),   psnr = mean_c 20 log10(1 / sqrt(mse_c))      the MEAN OF THE PER-CHANNEL PSNRs, as
 *   psnr(fake, target).mean() of heatmap.py:39 is (utils/image_utils.py:20-22), not the PSNR of the pooled error; mse_c = 0
 *   gives +inf.  metrics (B,2) f32 = [ssim, psnr]; ssim = the frame's d3ga_eval_ssim partials, added in index order in
 *   double, / (3 H W) (ssim_partials NULL: NaN is written);  psnr_channels (B,3) f32, optional;  accum: 3 doubles, optional,
 *   += [sum ssim, sum psnr, B] by float64 atomics (test.py:171-174 without a read-back per frame; needs ssim_partials, else
 *   D3GA_E_CONFIG).
 * d3ga_eval_partials: partials per (frame, channel) at this frame size, at most D3GA_EVAL_MAX_PARTIALS (< 0: D3GA_E_SIZE).
 * d3ga_eval_jet_table: the 257 x 3 uint8 table into HOST memory (row 256: the bad colour).
 *   Status, nothing launched: B, H, W <= 0, B > 65535 or H W > 2^26 D3GA_E_SIZE; an unknown flag, an output that has no
 *   meaning in the mode, or a tensor not aligned to its element (accum: 8 bytes) D3GA_E_CONFIG; pred or image NULL, alpha or
 *   boundary_fg NULL without D3GA_EVAL_COMPOSED, any pointer of d3ga_eval_ssim NULL, partials NULL in d3ga_eval_finish, or
 *   every output NULL D3GA_E_NULL.
 *   No scratch, no zero fill; capturable.
 * ------------------------------------------------------------------------------------------------------- */
#define D3GA_EVAL_BG_WHITE 1
#define D3GA_EVAL_COMPOSED 2
#define D3GA_EVAL_ALPHA3 4
#define D3GA_EVAL_BOUNDARY_F32 8
#define D3GA_EVAL_ALL 15
#define D3GA_EVAL_MAX_PARTIALS 2048
int d3ga_eval_frames(int32_t B, int32_t H, int32_t W, int32_t flags, const float *pred, const float *image, const float *alpha,
                     const void *boundary_fg, float *target_out, float *gt_out, float *heat_out, float *partials,
                     d3ga_stream_t stream);
int d3ga_eval_ssim(int32_t B, int32_t H, int32_t W, const float *pred, const float *target, float *ssim_partials,
                   d3ga_stream_t stream);
int d3ga_eval_finish(int32_t B, int32_t H, int32_t W, const float *partials, const float *ssim_partials, float *metrics,
                     float *psnr_channels, double *accum, d3ga_stream_t stream);
int64_t d3ga_eval_partials(int32_t H, int32_t W);
int64_t d3ga_eval_ssim_partials(int32_t H, int32_t W);
int d3ga_eval_jet_table(uint8_t *table);

/* ---------------------------------------------------------------------------------------------------------
 * Triangle-mesh rasterizer: the reference's recorder/mesh_renderer.py::Renderer (a pytorch3d MeshRasterizer with
 * blur_radius 0, one face per pixel, both windings, perspective-correct barycentrics, and HardFlatShader) for B meshes that
 * share one face list, one camera each.  Forward only.  Semantics: DESIGN.md 4.4f.
 *   verts (B,V,3) f32 world space;  faces (F,3) int32 (a face with an index outside [0, V) is dropped);
 *   cams (B,D3GA_MESH_CAM_FLOATS) f32: the world-to-camera rotation R row-major (9), t (3), fx, fy, cx, cy; OpenCV axes,
 *   x_cam = R x + t, u = fx x/z + cx, v = fy y/z + cy, pixel (column i, row j) samples (i + 0.5, j + 0.5).
 * d3ga_mesh_rasterize: a face with a vertex at z <= 0.01 or a doubled screen area below 1e-8 px^2 in magnitude is dropped.  Per
 *   pixel the face with the smallest zbuf = 1 / sum_i b_i / z_i wins, ties go to the smaller face index (a 64-bit unsigned
 *   atomic min over float_bits(zbuf) << 32 | face: bit-reproducible).  pix_to_face (B,H,W) int32, the index into `faces` or -1;
 *   zbuf (B,H,W) f32 and bary (B,H,W,3) f32 (perspective-correct), -1 where no face covers the pixel; both optional.
 *   scratch: d3ga_mesh_raster_scratch_bytes bytes, 16-byte aligned, contents irrelevant before the call (cleared by the call).
 *   Launches: clear, face setup, scan, coverage (a grid-stride loop over chunks whose total is read on the device), resolve.
 * d3ga_mesh_shade_flat: image (B,H,W,3) f32 from pix_to_face and bary: (0.45 + 0.35 max(n.l, 0)) texel + 0.05 [n.l > 0]
 *   max(v.r, 0)^64 with texel the interpolated verts_rgb (B,V,3) f32 (NULL: ones), n the face normal (not flipped), the light
 *   and the viewer at the camera centre; bg (3 floats, HOST memory, read by the call) where pix_to_face < 0.
 * d3ga_mesh_vertex_normals: normals (B,V,3) f32, the incident faces' cross(x1 - x0, x2 - x0) added in the order of the vertex's
 *   list, normalised with the norm clamped at 1e-6.  csr_offsets (V+1) int32, csr_faces (csr_offsets[V]) int32: the faces of
 *   each vertex (built once per face list by the caller; an entry outside [0, F) is skipped).  No atomics.
 * d3ga_mesh_maps: Renderer.map: position (B,H,W,3) f32 world, depth (B,H,W,1) f32 view z, normal (B,H,W,3) f32 =
 *   normalize(n_v0 + n_v1 + n_v2) of the winning face (norm clamped at 1e-8), mask (B,H,W,1) f32 = pix_to_face > 0 (so
 *   face 0 counts as background in the mask, as in the reference); all 0 where pix_to_face < 0.  Every output optional, not all.
 *   Status, nothing launched: a negative size, H or W outside [1, D3GA_MESH_MAX_SIDE] or B F >= 2^31 D3GA_E_SIZE; a required
 *   pointer NULL (verts with V > 0, faces with F > 0, ...) D3GA_E_NULL; a pointer not aligned to its element (scratch: 16 bytes)
 *   D3GA_E_CONFIG.  B = 0, V = 0 and F = 0 are valid (F = 0: background only).  No host synchronisation; capturable.
 * ------------------------------------------------------------------------------------------------------- */
#define D3GA_MESH_MAX_SIDE 16384
#define D3GA_MESH_CAM_FLOATS 16
int d3ga_mesh_raster_scratch_bytes(int32_t B, int32_t V, int32_t F, int32_t H, int32_t W, size_t *bytes);
int d3ga_mesh_rasterize(int32_t B, int32_t V, int32_t F, int32_t H, int32_t W, const float *verts, const int32_t *faces,
                        const float *cams, void *scratch, int32_t *pix_to_face, float *zbuf, float *bary, d3ga_stream_t stream);
int d3ga_mesh_shade_flat(int32_t B, int32_t V, int32_t F, int32_t H, int32_t W, const float *verts, const int32_t *faces,
                         const float *verts_rgb, const float *cams, const int32_t *pix_to_face, const float *bary, const float *bg,
                         float *image, d3ga_stream_t stream);
int d3ga_mesh_vertex_normals(int32_t B, int32_t V, int32_t F, const float *verts, const int32_t *faces, const int32_t *csr_offsets,
                             const int32_t *csr_faces, float *normals, d3ga_stream_t stream);
int d3ga_mesh_maps(int32_t B, int32_t V, int32_t F, int32_t H, int32_t W, const float *verts, const int32_t *faces,
                   const float *vertex_normals, const float *cams, const int32_t *pix_to_face, const float *bary, float *position,
                   float *normal, float *depth, float *mask, d3ga_stream_t stream);

/* pytorch3d's interpolate_face_attributes as the reference's Renderer.map runs it per frame (recorder/mesh_renderer.py:11,80-93):
 * pix_to_face (n_pix) int64 into packed faces, <0 = background; bary (n_pix,3); face_attrs (F_total,3,D) -> out (n_pix,D):
 *   out = b0*a0 + b1*a1 + b2*a2 in that order, f32, no contraction; background pixels get 0.
 * An index >= F_total writes 0 and reads nothing.  Forward only.  Status, nothing launched: a negative size
 * or D outside [1, D3GA_INTERP_MAX_D] D3GA_E_SIZE; a required pointer NULL (face_attrs with F_total > 0) D3GA_E_NULL; a pointer
 * not aligned to its element D3GA_E_CONFIG.  n_pix = 0 is valid.  No host synchronisation; capturable. */
#define D3GA_INTERP_MAX_D 64
int d3ga_interp_face_attrs(int64_t n_pix, int64_t F_total, int D, const int64_t *pix_to_face, const float *bary,
                           const float *face_attrs, float *out, d3ga_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Point-cloud view: the reference's recorder/pc_renderer.py::PCRenderer (a pytorch3d PointsRasterizer that keeps the K
 * nearest points of every pixel, + AlphaCompositor) for B clouds of P points, one camera each.  Forward only.  Semantics:
 * DESIGN.md 4.4h.
 *   points (B,P,3) f32 world space;  cams (B,D3GA_MESH_CAM_FLOATS) f32 as for the mesh rasterizer above, same projection and
 *   pixel centres;  radius: of a point's disc in NDC units, the shorter image side spanning [-1, 1] (radius min(H, W) / 2
 *   pixels);  K: points kept per pixel, 1 .. D3GA_POINTS_MAX_K.
 * d3ga_points_rasterize: a point at z <= 0.01 (or not finite) is dropped.  dist2 = ((i + 0.5 - u)^2 + (j + 0.5 - v)^2)
 *   (2 / min(H, W))^2; a point belongs to a pixel iff dist2 < radius^2.  Per pixel the K members with the smallest view depth
 *   z, equal depths by ascending index (the total order float_bits(z) << 32 | index: bit-reproducible, whatever the order of the
 *   points), nearest first: idx (B,H,W,K) int32, the index into the cloud, zbuf (B,H,W,K) f32 = z, dists (B,H,W,K) f32 = dist2;
 *   -1 in the empty slots; zbuf and dists optional.
 *   scratch: d3ga_points_raster_scratch_bytes bytes, 16-byte aligned, contents irrelevant before the call.  It holds the
 *   per-tile lists, sized by a closed-form bound on the 16 x 16 tiles a disc can touch: they cannot overflow.
 *   Launches: clear, count, two scans, scatter, one 256-lane workgroup per (view, tile).
 * d3ga_points_composite: image (B,H,W,3) f32 from idx and dists: sum_k w_k f_k prod_{j<k} (1 - w_j) over the filled slots with
 *   w_k = 1 - dists_k / radius^2 and f the point's colour, colors (B,P,3) f32 or NULL: (154, 205, 50) / 255; bg (3 floats, HOST
 *   memory, read by the call) only where slot 0 is empty: a covered pixel is not blended with the background.
 *   Status, nothing launched: a negative size, H or W outside [1, D3GA_MESH_MAX_SIDE], B P >= 2^31 or lists beyond 2^36
 *   records D3GA_E_SIZE; K outside [1, D3GA_POINTS_MAX_K] or a radius that is not positive and finite D3GA_E_CONFIG; a required
 *   pointer NULL (points with P > 0, cams, scratch, idx; idx, dists, bg, image) D3GA_E_NULL; a pointer not aligned to its
 *   element (scratch: 16 bytes) D3GA_E_CONFIG.  B = 0 and P = 0 are valid (P = 0: background only).  No host
 *   synchronisation; capturable.
 * ------------------------------------------------------------------------------------------------------- */
#define D3GA_POINTS_MAX_K 8
int d3ga_points_raster_scratch_bytes(int32_t B, int32_t P, int32_t H, int32_t W, float radius, size_t *bytes);
int d3ga_points_rasterize(int32_t B, int32_t P, int32_t H, int32_t W, int32_t K, float radius, const float *points,
                          const float *cams, void *scratch, int32_t *idx, float *zbuf, float *dists, d3ga_stream_t stream);
int d3ga_points_composite(int32_t B, int32_t P, int32_t H, int32_t W, int32_t K, float radius, const int32_t *idx,
                          const float *dists, const float *colors, const float *bg, float *image, d3ga_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Optimizer step, models/trainer.py:188-189: clip_grad_norm_(parameters, max_norm) + torch.optim.Adam.step() for every
 * parameter in THREE launches whatever the number of tensors (two with clipping off).  The tensors are described by tables
 * that the caller builds once per set of addresses, in device memory or in pinned host memory mapped to the device (read by
 * the kernels when they run, the chunk table once per call with clipping on: the form for a captured step, whose replays then
 * contain no copy node -- the host buffer must stay alive and unmodified as long as the graph is replayed):
 *   table         n_chunks records, one per run of at most D3GA_OPTIM_CHUNK consecutive elements of one tensor; the chunks
 *                 of a tensor need not be adjacent in the table.  flags & D3GA_OPTIM_ALIGNED16: p, g, m and v of the chunk
 *                 are all 16-byte aligned (16-byte loads and stores; otherwise element by element).
 *   tensor_state  n_tensors records: `step`, ONE float32 in device memory (torch.optim.Adam's state["step"]), read,
 *                 incremented and written back by the call; `group` indexes group_hparams.
 *   group_hparams n_groups x 4 doubles in DEVICE memory: lr, beta1, beta2, eps.  Read when the kernels run, so a captured
 *                 step follows a learning-rate schedule by overwriting them.
 * With N = sqrt(sum over all chunks of g^2):
 *     clip_coef = min(1, max_norm / (N + 1e-6))                      (max_norm < 0: no clipping, N is not computed)
 *     g' = clip_coef g;  m = beta1 m + (1 - beta1) g';  v = beta2 v + (1 - beta2) g'^2
 *     p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * g is only read (the gradients stay unclipped).  grad_norm_out: one float32 in device memory receiving N (NULL: skipped;
 * untouched without clipping).  N is summed without atomics in a fixed order (per chunk in float32; the chunks in double, thread t of one workgroup taking chunks t, t + 256, ... and an LDS tree over
 * the 256 threads): bit-identical from run to run.  Non-finite gradients propagate as in the reference.
 * scratch: d3ga_optim_scratch_bytes() bytes, 256-byte aligned, contents irrelevant.
 * ------------------------------------------------------------------------------------------------------- */
#define D3GA_OPTIM_CHUNK 8192
#define D3GA_OPTIM_ALIGNED16 1
typedef struct d3ga_optim_chunk { /* 48 bytes */
    float *p;                     /* parameter   (read, written) */
    const float *g;               /* gradient    (read) */
    float *m;                     /* exp_avg     (read, written) */
    float *v;                     /* exp_avg_sq  (read, written) */
    int32_t n;                    /* elements, 1 .. D3GA_OPTIM_CHUNK */
    int32_t tensor;               /* index into tensor_state */
    int32_t flags;                /* D3GA_OPTIM_ALIGNED16 */
    int32_t reserved;
} d3ga_optim_chunk;
typedef struct d3ga_optim_tensor { /* 16 bytes */
    float *step;
    int32_t group;
    int32_t reserved;
} d3ga_optim_tensor;
int d3ga_optim_scratch_bytes(int32_t n_chunks, int32_t n_tensors, int32_t n_groups, int64_t *out); /* host only */
int d3ga_optim_clip_adam_step(const d3ga_optim_chunk *table, int32_t n_chunks, const d3ga_optim_tensor *tensor_state,
                              int32_t n_tensors, const double *group_hparams, int32_t n_groups, float max_norm,
                              void *scratch, float *grad_norm_out, d3ga_stream_t stream);

/* Test hook, not part of the drop-in surface: the 16-lane DPP row scans of the compositing backward.  n multiple of
 * 256; in (n) -> out (8n): for element i (lane l of its row), out[8i+k] = sum over lanes <= l of (k+1) in, k < 4, and
 * out[8i+4+k] = product over lanes <= l of (1 + (k+1)/8 in). */
int d3ga_selftest_row_scan(int n, const float *in, float *out, d3ga_stream_t stream);
/* Test hook, not part of the drop-in surface: the compositing forward's own alpha evaluation (and its "touches the pixel"
 * decision: power <= 0 and alpha >= 1/255) for n listed pairs (Gaussian gid[i], pixel (px[i], py[i])) over the geometry
 * records `geom` of a forward with P Gaussians.  ok (n) u8; alpha (n) f32 or NULL.  Lets a parity test share the product's
 * threshold decisions with the oracle (tests/test_gpu_parity.py: shared decisions). */
int d3ga_selftest_alpha(int32_t P, const void *geom, int n, const int32_t *gid, const int32_t *px, const int32_t *py,
                        uint8_t *ok, float *alpha, d3ga_stream_t stream);

/* Init-time point location: for each of P points the tet (of T, corners (T,4,3)) with the largest minimum barycentric weight,
 * the lowest index among equals (csrc/bary_math.h); active = that minimum >= 0.  A tet whose volume evaluates to 0 or whose
 * weights are not finite is never chosen; if none can be, the row is (0, 0, 0).  barys (P,4) is stored 16 bytes at a time:
 * D3GA_E_CONFIG unless it is 16-byte aligned (d3ga_compute_bary_grid as well). */
int d3ga_compute_bary(int P, int T, const float *points, const float *tetra_corners, float *barys,
                      int32_t *tetra_id, uint8_t *active, d3ga_stream_t stream);

/* The same search with uniform-grid candidate pruning (bit-identical results for points inside the
 * cage).  cell_start (nx*ny*nz + 1) / cell_tets: per grid cell the tets whose bounding box overlaps it (CSR, int32);
 * origin_h = {ox, oy, oz, cell edge} (HOST array), dims = {nx, ny, nz} (HOST array).  min_weight (P) receives the
 * winner's smallest weight: < 0 means no candidate contains the point -- re-run those through d3ga_compute_bary. */
int d3ga_compute_bary_grid(int P, const float *points, const float *tetra_corners, const int32_t *cell_start,
                           const int32_t *cell_tets, const float *origin_h, const int32_t *dims, float *barys,
                           int32_t *tetra_id, float *min_weight, d3ga_stream_t stream);

/* Init-time scale seed.  Replaces simple_knn._C.distCUDA2 (models/mesh_net.py:22,66) and
 * pytorch3d knn_points(p, p, K=4)[0][0,:,1:].mean(-1) (models/cage_net.py:66): out[i] = mean squared distance of
 * point i to its 3 nearest other points (sum / 3; missing neighbours count as 0, like pytorch3d's padding).  points (P,3) -> out (P).
 * The squared distance is d3ga_knn_points' (csrc/knn_math.h: knn_dist2), so the two forms agree up to the rounding of the mean.
 * A point with a coordinate that is not finite gets 0 and is nobody's neighbour.  Exhaustive O(P^2). */
int d3ga_knn3_mean_dist2(int P, const float *points, float *out, d3ga_stream_t stream);
/* The same with a uniform grid over the points (cell_start / cell_points: CSR of point indices per cell; origin_h, dims as
 * above, HOST arrays): ring search outwards from the point's cell, exact. */
int d3ga_knn3_mean_dist2_grid(int P, const float *points, const int32_t *cell_start, const int32_t *cell_points,
                              const float *origin_h, const int32_t *dims, float *out, d3ga_stream_t stream);

/* K nearest neighbours with distances and indices: pytorch3d's knn_points as models/cage_net.py:21,66 calls it
 * (knn_points(points[None], points[None], K = 4)), forward only.  Semantics (specification of record):
 * the squared distance is dx*dx + dy*dy + dz*dz in f32 without contraction, plus the first-order term of what the three f32
 * subtractions lost (0 where they are exact; csrc/knn_math.h: within 4 * 2^-24 d of the distance of the f32 coordinates); neighbours are ordered by the
 * pair (distance, index), the lower index first on equal distances, so the result does not depend on the order of the search;
 * a query that is itself in p2 finds itself; with P2 < K the missing slots are dists = 0, idx = 0 (pytorch3d's padding).
 *   p1 (N,P1,3), p2 (N,P2,3) f32 -> dists (N,P1,K) f32 squared distances ascending, idx (N,P1,K) int64 into p2.  Exhaustive. */
#define D3GA_KNN_MAX_K 16
int d3ga_knn_points(int N, int P1, int P2, int K, const float *p1, const float *p2, float *dists, int64_t *idx, d3ga_stream_t s);
/* one batch element, p2 bucketed in a uniform grid (CSR as d3ga_knn3_mean_dist2_grid takes it; origin_h, dims HOST arrays):
 * exact ring search, bit-identical to d3ga_knn_points.  The queries need not be members of p2 nor lie inside its box.
 * Status of both, nothing launched: a negative size, N > 65535, K outside [1, D3GA_KNN_MAX_K], a dimension < 1, a cell edge
 * that is not positive and finite D3GA_E_SIZE; a required pointer NULL (p2, cell_points with P2 > 0) D3GA_E_NULL.  P1 = 0 or
 * N = 0: D3GA_OK without a launch. */
int d3ga_knn_points_grid(int P1, int P2, int K, const float *p1, const float *p2, const int32_t *cell_start,
                         const int32_t *cell_points, const float *origin_h, const int32_t *dims,
                         float *dists, int64_t *idx, d3ga_stream_t s);

/* ---------------------------------------------------------------------------------------------------------
 * Field networks: the dense layer of models/mlp.py:39-232 -- every field is
 * z -> [Linear(128) + leaky_relu(0.1)] x (1 + n_layers) -> Linear -- on the matrix cores with f32-equivalent accuracy:
 * every f32 operand is split exactly into three bf16 pieces and the six leading cross products are accumulated in f32
 * (v_mfma_f32_32x32x16_bf16); the dropped products are below 2^-24 |x||w|, the rounding of an f32 fmaf chain.
 *   Y (P, n_out) = act_out( X (P,K) . W + bias ),  act_out(y) = y > 0 ? y : out_slope * y   (out_slope = 1: identity)
 *   sign_out (P, ceil(n_out/32)) uint32, optional: bit (n & 31) of word [r][n >> 5] = (Y[r][n] > 0) -- all the backward
 *   needs of a leaky_relu output.
 *   mask_bits (same layout), optional:  Y (.)= (bit ? 1 : mask_slope)  -- the backward chain: X = dPre of a layer, W its
 *   transposed weights, mask_bits = the sign bits of the layer below, so that Y is THAT layer's dPre (the operand of
 *   its weight gradient dW = dPre^T . input and of the next call); no masked copy is ever written.
 *   panel: the split weights in the kernel's operand order, d3ga_mlp_panel_bytes(K, n_out) bytes, written by
 *   d3ga_mlp_pack_weights from plain f32 weights: weight of input k for output n = W[k*ld_k + n*ld_n]
 *   (an nn.Linear weight (n_out,K): ld_k = 1, ld_n = K; the input-gradient GEMM of the same layer contracts over the
 *   layer's outputs: K := n_out, n_out := K, ld_k = K_layer, ld_n = 1).  Re-pack whenever the weights change.
 *   K <= 128, n_out <= 128; X, panel 16-byte aligned.  bias may be NULL.
 * ------------------------------------------------------------------------------------------------------- */
int64_t d3ga_mlp_panel_bytes(int32_t K, int32_t n_out);          /* < 0: D3GA_E_SIZE */
int d3ga_mlp_pack_weights(int32_t K, int32_t n_out, const float *W, int64_t ld_k, int64_t ld_n, void *panel,
                          d3ga_stream_t stream);
int d3ga_mlp_linear(int32_t P, int32_t K, int32_t n_out, const float *X, const void *panel, const float *bias,
                    float out_slope, uint32_t *sign_out, const uint32_t *mask_bits, float mask_slope, float *Y,
                    d3ga_stream_t stream);

/* One launch for a whole trunk (forward): h_{l+1} = act_l(h_l W_l^T + b_l), l = 0..L-1, with the activations kept in the
 * registers of the wavefront that owns the rows -- no activation is read back between the layers.  Same
 * arithmetic as d3ga_mlp_linear (exact 3-way bf16 split, six products, f32 accumulate).  Layer l: Ks[l] inputs (= Ns[l-1];
 * Ks[0] = K0 <= 128), Ns[l] <= 128 outputs, panels[l] = its weights packed by d3ga_mlp_pack_chain (d3ga_mlp_chain_panel_bytes;
 * the call writes biases[l] -- or zeros: biases / biases[l] may be NULL -- into the 512-byte tail of panels[l], which is why
 * the panels are not const), leaky_relu slope slopes[l] (1 = none) applied to its output; outs[l] (P, Ns[l]) receives that output and
 * signs[l] (or NULL) one bit per output element (P, ceil(Ns[l]/32)) words, bit c of word b = out[row][32 b + c] > 0 before the
 * slope -- exactly what d3ga_mlp_linear writes, so the per-layer backward applies unchanged.  L <= 8.
 * The same launch runs the BACKWARD's input-gradient chain: X = the gradient at the trunk's output, panels[l] = the transposed
 * weights (d3ga_mlp_pack_chain with ld_k / ld_n swapped, bias NULL), slopes[l] = 1, masks[l] (or NULL; masks itself may be
 * NULL) = the sign words the forward wrote for the layer BELOW output l: outs[l] (.)= bit ? 1 : mask_slopes[l] -- outs[l] is
 * then that layer's pre-activation gradient (d3ga_mlp_linear's mask_bits); a call with masks must have no bias, no activation
 * (slopes 1) and no sign output on any layer.  Supported shapes: L >= 2, every layer but the
 * last 128 wide, K0 <= 128, the last one <= 128 wide; D3GA_E_CONFIG otherwise (use d3ga_mlp_linear). */
int64_t d3ga_mlp_chain_panel_bytes(int32_t K, int32_t n_out);
int d3ga_mlp_pack_chain(int32_t K, int32_t n_out, const float *W, int64_t ld_k, int64_t ld_n, void *panel, d3ga_stream_t stream);
int d3ga_mlp_chain_fwd(int32_t P, int32_t K0, const float *X, int32_t L, const int32_t *Ks, const int32_t *Ns,
                       void *const *panels, const float *const *biases, const float *slopes, float *const *outs,
                       uint32_t *const *signs, const uint32_t *const *masks, const float *mask_slopes, d3ga_stream_t stream);
/* Weight and bias gradient of that layer: dW (N,K) = dPre^T . X, db (N) = column sums of dPre (db may be NULL);
 * dPre (P,N) = the gradient at the layer's pre-activation (see above), X (P,K) the layer's input.  Both outputs are zeroed by the call; partial sums meet through float atomics. */
int d3ga_mlp_wgrad(int32_t P, int32_t N, int32_t K, const float *dpre, const float *X, float *dW, float *db,
                   d3ga_stream_t stream);
/* Same, accumulating: dW += dPre^T . X, db += column sums; nothing is zeroed (a chain of layers zeroes ONE flat buffer
 * for all its weight gradients instead of two memsets per layer). */
int d3ga_mlp_wgrad_acc(int32_t P, int32_t N, int32_t K, const float *dpre, const float *X, float *dW, float *db,
                       d3ga_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * The element-wise ops in front of ColorField.
 *   view_dirs:     dirs (P,3) = (means3D - campos) / |means3D - campos|          models/cage_net.py:233-235
 *   sh4_encoding:  enc (P,16) = real spherical harmonics of degree < 4 on x = 2 dirs - 1: the degree-4
 *                  "SphericalHarmonics" direction encoding of models/mlp.py:166-179 (tiny-cuda-nn, un-vendored:
 *                  restated from its published definition, constants of utils/sh_utils.py:7-24).
 * The backward calls overwrite d_means3D / d_dirs (no accumulation).  enc, d_enc 16-byte aligned.
 * ------------------------------------------------------------------------------------------------------- */
/* Output heads of a field network (models/mlp.py:107-110, 232): pred (P,N) -> n_heads <= 4 consecutive column groups of
 * widths width[h] (sum = N), head h written as a contiguous (P, width[h]) block at out + P * (width[0] + .. + width[h-1])
 * through act[h]: 0 identity, 1 param[h] * tanh(x), 2 sigmoid(x + param[h]).  width, act, param are HOST arrays.
 * bwd: d_pred (P,N) from the heads' gradients g0..g3 (each (P, width[h]) contiguous, NULL = unused head -> zero) and the
 * forward's `out`. */
int d3ga_field_heads_fwd(int32_t P, int32_t N, int32_t n_heads, const int32_t *width, const int32_t *act, const float *param,
                         const float *pred, float *out, d3ga_stream_t stream);
int d3ga_field_heads_bwd(int32_t P, int32_t N, int32_t n_heads, const int32_t *width, const int32_t *act, const float *param,
                         const float *out, const float *g0, const float *g1, const float *g2, const float *g3, float *d_pred,
                         d3ga_stream_t stream);
int d3ga_view_dirs_fwd(int32_t P, const float *means3D, const float *campos, float *dirs, d3ga_stream_t stream);
int d3ga_view_dirs_bwd(int32_t P, const float *means3D, const float *campos, const float *d_dirs, float *d_means3D,
                       d3ga_stream_t stream);
int d3ga_sh4_encoding_fwd(int32_t P, const float *dirs, float *enc, d3ga_stream_t stream);
int d3ga_sh4_encoding_bwd(int32_t P, const float *dirs, const float *d_enc, float *d_dirs, d3ga_stream_t stream);
/* ColorField's per-row input columns in one pass (models/mlp.py:208-226: z's per-row groups when no shadow column is present):
 * x (P, 16 + F) = [ sh4_encoding(dirs) | feats (P,F) ], F a multiple of 4, x / feats 16-byte aligned -- instead of the encoding
 * call and a torch.cat; backward: d_x (P, 16 + F) -> d_dirs (P,3) and d_feats (P,F), either may be NULL (ABI 104). */
int d3ga_color_rows_fwd(int32_t P, int32_t F, const float *dirs, const float *feats, float *x, d3ga_stream_t stream);
int d3ga_color_rows_bwd(int32_t P, int32_t F, const float *dirs, const float *d_x, float *d_dirs, float *d_feats,
                        d3ga_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * B2  Goliath skeleton (added without an ABI number change: new entry points only, no existing layout moves).
 * The momentum-style skeleton of lbsmodel/body_model.py: ParameterTransform (:23-46), solve_skeleton_state (:311-347),
 * states_to_matrix (:350-387) and the root transform (:176-191).  Host side: d3ga_amd/skeleton_model.py.
 *   A skeleton state is 8 floats: translation 3 | quaternion xyzw 4 | scale 1.  Quaternions are used as given (never normalised;
 *   the bind inverse divides by |q|^2).
 *   Every joint has 7 skeleton parameters [t 3 | Euler xyz 3 | log2 scale] = transform . [poses; scales] + transform_offsets;
 *   the (7J, n_params) transform is held twice, nonzeros only: CSR (csr_ptr (7J+1), csr_col ascending, csr_val) for the forward
 *   and CSC (csc_ptr (n_params+1), csc_row ascending, csc_val) for its transpose in the backward.
 *   Local transform: t + joint_offset, joint_rotation (x) q(Euler) with half angles (-rx/2, ry/2, rz/2), scale 2^p.
 *   Child from parent: q = q_p (x) q_l, t = rot(q_p, t_l s_p) + t_p, s = s_p s_l; parents[j] < 0 is a root (its state is its
 *   local transform).  The tree by level (level_ptr (n_levels+1), level_joint (J): a parent sits in an earlier level) and by
 *   children (child_ptr (J+1), child_joint (n_children), a joint's children ascending).  2 <= J <= D3GA_SKEL_MAX_JOINTS.
 *   Joint matrix against a bind state (J,8): [R(q (x) q_b^-1) s / s_b | t], written as the row-major 4x4 d3ga_lbs_cage_fwd reads,
 *   its translation column multiplied by trans_scale (a unit change folded into the skinning; the root output is not scaled).
 * fwd: one workgroup per (frame, scale set).  poses (B, pose_width) are parameters 0 .. pose_width, scales the remaining
 *   n_params - pose_width ones: (scale_rows, .) with scale_rows 1 (shared by the frames) or B, NULL = zeros.  Scale set 0 reads
 *   `scales`, sets 1 .. n_sets-1 read zeros (the root solve of LinearBlendSkinning.compute_root_rigid_transform).  direct != NULL:
 *   (B, 7J) skeleton parameters as they are, no transform (n_sets must be 1).
 *   -> states (n_sets,B,J,8), saved (n_sets,B,J,D3GA_SKEL_SAVED_FLOATS) for the backward, mats (n_sets,B,J,4,4) | NULL,
 *   root (n_sets,B,12) = [R 9 row-major | t 3] of joint root_joint | NULL; mats and root need bind.
 * bwd: one workgroup per frame.  Upstream g_states, g_mats (bottom row ignored), g_root in the forward's layouts, NULL = zero
 *   -> g_poses (B, pose_width), g_scales (B, n_params - pose_width) per frame (from set 0 only), or with direct_mode
 *   g_direct (B, 7J); NULL = not written.  No atomics: two calls give bitwise-equal gradients.
 * No scratch, no host synchronisation: capturable.  d3ga_skeleton_check: the host-side size / NULL checks of both.
 * ------------------------------------------------------------------------------------------------------- */
#define D3GA_SKEL_MAX_JOINTS 512
#define D3GA_SKEL_SAVED_FLOATS 12       /* per joint: local state 8 | Euler angles 3 | 0 */
typedef struct d3ga_skeleton {
    int32_t J, n_params;        /* joints; pose + scale parameters */
    int32_t n_levels;           /* levels of the kinematic tree */
    int32_t n_children;         /* joints with a parent */
    const int32_t *parents, *level_ptr, *level_joint, *child_ptr, *child_joint;
    const float *joint_offset;      /* (J,3) */
    const float *joint_rotation;    /* (J,4) xyzw */
    const float *transform_offsets; /* (7J) */
    const int32_t *csr_ptr, *csr_col;
    const float *csr_val;
    const int32_t *csc_ptr, *csc_row;
    const float *csc_val;
} d3ga_skeleton;
int d3ga_skeleton_check(const d3ga_skeleton *model, int32_t B, int32_t n_sets, int32_t pose_width);
int d3ga_skeleton_fwd(const d3ga_skeleton *model, int32_t B, int32_t n_sets, int32_t pose_width, const float *poses,
                      const float *scales, int32_t scale_rows, const float *direct, const float *bind, float trans_scale,
                      int32_t root_joint, float *states, float *saved, float *mats, float *root, d3ga_stream_t stream);
int d3ga_skeleton_bwd(const d3ga_skeleton *model, int32_t B, int32_t n_sets, int32_t pose_width, int32_t direct_mode,
                      const float *bind, float trans_scale, int32_t root_joint, const float *states, const float *saved,
                      const float *g_states, const float *g_mats, const float *g_root, float *g_poses, float *g_scales,
                      float *g_direct, d3ga_stream_t stream);
/* states (B,J,8) -> mats (B,J,4,4) against bind (J,8), and dL/d(states) from g_mats (bottom row ignored; bind is a constant) */
int d3ga_skeleton_mats_fwd(int32_t B, int32_t J, const float *bind, const float *states, float *mats, d3ga_stream_t stream);
int d3ga_skeleton_mats_bwd(int32_t B, int32_t J, const float *bind, const float *states, const float *g_mats, float *g_states,
                           d3ga_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * VGG19 perceptual loss.  Replaces utils/loss_utils.py:109-160 VGGLoss (train.py:212-214): the 2x2 box downsize,
 * conv1_1 .. conv5_1 with ReLU and four 2x2 max pools, and an L1 mean per feature tap (d3ga_l1_mean_fwd_ws / _bwd above).
 * The weights are frozen: only input gradients exist.  Activations are channels-last (H, W, C) float32; the image is (C, H, W).
 * No entry point allocates or synchronises; all are capturable.  Every size is checked before any launch: H, W, C >= 1 and
 * H W C <= INT32_MAX (else D3GA_E_SIZE), required pointers (D3GA_E_NULL), alignment and flags (D3GA_E_CONFIG).
 *
 * d3ga_vgg_panel_bytes(cin, cout): bytes of the packed weights of a convolution GEMM with cin inputs and cout outputs (three
 *   bf16 planes, K and N padded to the MFMA tile; csrc/perceptual_math.h has the slot map).  < 0: D3GA_E_SIZE.
 * d3ga_vgg_pack_weights: weight (w_cout, w_cin, 3, 3) -> panel, once per weight set.  transposed = 0: the forward panel
 *   (d3ga_vgg_panel_bytes(w_cin, w_cout)); transposed = 1: the flipped, transposed panel of the input gradient
 *   (d3ga_vgg_panel_bytes(w_cout, w_cin)).  panel 16-byte aligned.
 * d3ga_vgg_conv3x3: y (H,W,cout) = [accumulate ? y : 0] + act( conv3x3(x', panel) + bias ), stride 1, zero padding 1, with
 *   x' = x (H,W,cin), or x (.) [mask_y > 0] when mask_y (H,W,cin) is given; act = ReLU when relu = 1; bias (cout) | NULL.
 *   Forward: (x, NULL, forward panel, bias, relu 1).  Input gradient of the layer that produced Y: (dY, Y, transposed panel,
 *   NULL, relu 0) with cin = the layer's output width.  f32-equivalent arithmetic (three-piece bf16 split, six products).
 *   x, mask_y, panel 16-byte aligned; y must not alias x or mask_y (D3GA_E_CONFIG).
 * d3ga_vgg_maxpool2_fwd / _bwd: 2x2, stride 2, floor; x (H,W,C) -> y (H/2,W/2,C); gx (H,W,C) from gy: the window's first
 *   maximum in row-major order takes the gradient (torch's rule), the dropped odd row / column exact zeros.  H, W >= 2.
 * d3ga_vgg_box_down2_fwd / _bwd: img (C,H,W) -> out (H/2,W/2,C) = the 2x2 box mean of img[:, :2(H/2), :2(W/2)] -- what
 *   F.interpolate(scale_factor=0.5, mode="bilinear") computes -- or, with down = 0, the transpose to channels-last alone (the
 *   reference passes a 512 x 512 image unchanged).  bwd: g (out's shape) -> g_img (C,H,W), zeros in a dropped row / column.
 * d3ga_vgg_scratch_bytes (host): for a (3,H,W) image, halved first by d3ga_vgg_box_down2_fwd if down = 1, n_layers taps (1..5, else D3GA_E_CONFIG) and 13 conv widths (NULL:
 *   VGG19's), out[0] = bytes of the source activations and per-tap L1 gradients kept for the backward, out[1] = bytes of the forward's work area
 *   (target ping-pong, D3GA_LOSS_PARTIALS, tap means), out[2] = bytes of the backward's gradient ping-pong; every tensor
 *   inside starts on a 256-byte boundary, in the order d3ga_amd/perceptual.py carves them.  An image too small for the
 *   pools of the chain: D3GA_E_SIZE.
 * ------------------------------------------------------------------------------------------------------- */
int64_t d3ga_vgg_panel_bytes(int32_t cin, int32_t cout);
int d3ga_vgg_pack_weights(int32_t w_cout, int32_t w_cin, const float *weight, int32_t transposed, void *panel,
                          d3ga_stream_t stream);
int d3ga_vgg_conv3x3(int32_t H, int32_t W, int32_t cin, int32_t cout, const float *x, const float *mask_y, const void *panel,
                     const float *bias, int32_t relu, int32_t accumulate, float *y, d3ga_stream_t stream);
int d3ga_vgg_maxpool2_fwd(int32_t H, int32_t W, int32_t C, const float *x, float *y, d3ga_stream_t stream);
int d3ga_vgg_maxpool2_bwd(int32_t H, int32_t W, int32_t C, const float *x, const float *gy, float *gx, d3ga_stream_t stream);
int d3ga_vgg_box_down2_fwd(int32_t C, int32_t H, int32_t W, int32_t down, const float *img, float *out, d3ga_stream_t stream);
int d3ga_vgg_box_down2_bwd(int32_t C, int32_t H, int32_t W, int32_t down, const float *g, float *g_img, d3ga_stream_t stream);
int d3ga_vgg_scratch_bytes(int32_t H, int32_t W, int32_t down, int32_t n_layers, const int32_t *widths, int64_t *out);
/* The same convolution and pool over N images (N,H,W,C) at once: the images ride in the GEMM's M dimension and share every
 * weight load; the zero padding is per image (no tap reads across a seam).  Every other argument as above; the size rule is
 * N H W C <= INT32_MAX.  Image n of the result is bit for bit what the single-image call gives on image n; the single-image
 * entry points are the N = 1 case of the same kernels.  d3ga_vgg_maxpool2_fwd_n: y must not be x (D3GA_E_CONFIG). */
int d3ga_vgg_conv3x3_n(int32_t N, int32_t H, int32_t W, int32_t cin, int32_t cout, const float *x, const float *mask_y,
                       const void *panel, const float *bias, int32_t relu, int32_t accumulate, float *y, d3ga_stream_t stream);
int d3ga_vgg_maxpool2_fwd_n(int32_t N, int32_t H, int32_t W, int32_t C, const float *x, float *y, d3ga_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * LPIPS (VGG), forward only: the third metric of recorder/heatmap.py:13, 40.  The chain is VGG16 -- 13 convolutions
 * (d3ga_vgg_conv3x3_n), a pool (d3ga_vgg_maxpool2_fwd_n) in front of conv index 2, 4, 7, 10, a tap behind conv index 1, 3, 6,
 * 9, 12 -- with fake and target as one batch of 2 B images; csrc/lpips_math.h states the arithmetic.  No entry point
 * allocates or synchronises; all are capturable; sizes (D3GA_E_SIZE), pointers (D3GA_E_NULL), alignment, flags and
 * overlapping buffers (D3GA_E_CONFIG) are refused before any launch.  No float atomics: results are reproducible bit for bit.
 *
 * d3ga_lpips_input: img (N,3,H,W) -> out (N,H,W,3) = ((normalize ? 2 x - 1 : x) - shift_c) / scale_c,
 *   shift = (-.030, -.088, -.188), scale = (.458, .448, .450).
 * d3ga_lpips_tap: features a, b (B,h,w,C), 1 <= C <= 512, weights lin (C), any sign:
 *     d(p) = sum_c lin_c (a_c / (|a| + 1e-10) - b_c / (|b| + 1e-10))^2,  |a| = sqrt(sum_c a_c^2)
 *   (the difference before the square: a == b gives exactly 0; an all-zero vector contributes 0, not NaN) -> map (B,h,w) | NULL,
 *   and value[b] = [accumulate ? value[b] : 0] + mean_p d(p) through `partials`, B * D3GA_LPIPS_PARTIALS floats of scratch, in
 *   two stages of a fixed order: image b of a batch is bit for bit the single-pair call.  a may be b.
 * d3ga_lpips_scratch_bytes (host): the work area of B image pairs (3,H,W), H, W >= 16 (four floor pools; else D3GA_E_SIZE),
 *   with 13 conv widths (NULL: VGG16's; a tap wider than 512: D3GA_E_SIZE): out[0] = all of it = 2 out[1] + out[2],
 *   out[1] = one buffer of the activation ping-pong (the widest layer of the 2 B images), out[2] = the partials; each part
 *   starts on a 256-byte boundary in that order.  A tap's features are consumed before the buffers rotate.
 * ------------------------------------------------------------------------------------------------------- */
#define D3GA_LPIPS_PARTIALS 1024
int d3ga_lpips_input(int32_t N, int32_t H, int32_t W, int32_t normalize, const float *img, float *out, d3ga_stream_t stream);
int d3ga_lpips_tap(int32_t B, int32_t h, int32_t w, int32_t C, const float *a, const float *b, const float *lin, float *map,
                   float *partials, float *value, int32_t accumulate, d3ga_stream_t stream);
int d3ga_lpips_scratch_bytes(int32_t B, int32_t H, int32_t W, const int32_t *widths, int64_t *out);

/* ---------------------------------------------------------------------------------------------------------
 * Per-frame state addressed by a device index: the frame codes and the refined SMPL-X parameters of
 * models/garment_net.py:87-107, 163-178, 211-235, so that a captured step follows the frame of every replay.  No entry point
 * allocates or synchronises; all are capturable; no atomics, every sum in a fixed order: results are reproducible bit for bit.
 *
 * d3ga_code_lookup_fwd: models/embeddings.py:31-36 over nn.Embedding(max_norm).  table (N,D), idx (B) int32 ON THE DEVICE, each
 *   clamped into [0, N-1] (the reference clamps the top only) -> out (B,D).  First torch's embedding_renorm_, IN PLACE on
 *   table: every distinct looked-up row whose L2 norm is > max_norm (strictly) is multiplied by max_norm / (norm + 1e-7);
 *   max_norm <= 0: no renorm.  Then the rows are copied.  A row named several times is renormed once and all its copies in
 *   out are equal.  One launch.  1 <= B <= D3GA_CODE_MAX_B, 1 <= D <= D3GA_CODE_MAX_D, N D <= INT32_MAX, else D3GA_E_SIZE.
 * d3ga_code_lookup_bwd: dout (B,D) -> dtable (N,D), the dense gradient nn.Embedding produces.  EVERY element is written: the sum
 *   of dout[b] over the b with idx[b] = row, in increasing b; zero for a row nobody names (no separate clear).  One launch.
 * d3ga_table_mean: Embedding.average(): out (D) = the mean of table (N,D) over its rows, summed in float64 in two stages of a
 *   fixed order (two launches) through `scratch`, d3ga_table_mean_scratch_bytes(N, D) bytes, 8-byte aligned (else D3GA_E_CONFIG).
 * d3ga_row_cache_select: desc (HOST, copied into the launch) lists n_pairs <= D3GA_ROW_CACHE_MAX_PAIRS pairs of a table
 *   (n_rows, width) and a stage (width) of 4-byte words; idx, prev, flag: one int32 each on the device.  In one launch:
 *     1. if prev >= 0, every stage is copied back into row prev of its table;  2. row idx of every table is copied into its
 *     stage;  3. prev = idx.
 *   idx == prev changes nothing.  idx outside [0, n_rows) of ANY pair (or a prev that is not -1 or a row): nothing moves, prev
 *   stays, and flag is set to 1 (sticky: nobody clears it but the caller).
 * d3ga_row_cache_flush: step 1 alone; prev stays.
 * ------------------------------------------------------------------------------------------------------- */
#define D3GA_CODE_MAX_B 16
#define D3GA_CODE_MAX_D 4096
#define D3GA_TABLE_MEAN_CHUNKS 64
#define D3GA_ROW_CACHE_MAX_PAIRS 16
typedef struct d3ga_row_pair {
    float *table;
    float *stage;
    int32_t width;
    int32_t n_rows;
} d3ga_row_pair;
int d3ga_code_lookup_fwd(float *table, const int32_t *idx, int32_t N, int32_t D, int32_t B, float max_norm, float *out,
                         d3ga_stream_t stream);
int d3ga_code_lookup_bwd(const float *dout, const int32_t *idx, int32_t N, int32_t D, int32_t B, float *dtable,
                         d3ga_stream_t stream);
int d3ga_table_mean_scratch_bytes(int32_t N, int32_t D, int64_t *bytes);
int d3ga_table_mean(const float *table, int32_t N, int32_t D, float *out, void *scratch, d3ga_stream_t stream);
int d3ga_row_cache_select(const d3ga_row_pair *desc, int32_t n_pairs, const int32_t *idx, int32_t *prev, int32_t *flag,
                          d3ga_stream_t stream);
int d3ga_row_cache_flush(const d3ga_row_pair *desc, int32_t n_pairs, int32_t *prev, int32_t *flag, d3ga_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * The training objective: the scale regulariser of models/cage_net.py:214, 226 and the block of train.py:190-244
 * that turns the per-frame losses and regularisers into the weighted total, with the NaN test of train.py:64-69 left on the
 * device.  No entry point allocates or synchronises; all are capturable; no atomics, every sum in a fixed order (written down
 * in csrc/objective_math.h): results are reproducible bit for bit.
 *
 * d3ga_scale_energy_fwd: out[0] = (1/n) sum_i act(scaling_i + delta_i)^2 over n floats (delta NULL: 0); activation
 *   D3GA_SCALE_ACT_EXP | D3GA_SCALE_ACT_NONE (else D3GA_E_CONFIG).  Two launches: one partial sum per workgroup into `partials`
 *   (>= D3GA_LOSS_PARTIALS floats, contents irrelevant), then one workgroup adds them in index order.  scaling and delta
 *   16-byte aligned (else D3GA_E_CONFIG).
 * d3ga_scale_energy_bwd: grad_i = g[0] * d/dx act(x_i)^2 / n with x = scaling + delta, the activation recomputed: the ONE array
 *   both inputs receive.  g on the device.  One launch; grad 16-byte aligned too.
 * d3ga_objective_fwd: desc (HOST, copied into the launch: the table of pointers and lengths travels in the kernel arguments,
 *   as d3ga_row_cache_select's does) lists, for each of 1 <= n_frames <= D3GA_OBJ_MAX_FRAMES frames, D3GA_OBJ_SLOTS entries in
 *   the order l1, ssim, sil_l1 (1 float each), scale_energy (n_cages), fm_energy (n_cages | absent), frame_encoding (D),
 *   optimizable_poses (N | absent), blur_weights (n | absent), vgg (1 | absent); an absent entry has ptr NULL, and every frame
 *   must have the same entries present with the same lengths of scale_energy and fm_energy (else D3GA_E_CONFIG); lengths
 *   1..D3GA_OBJ_MAX_LEN (else D3GA_E_SIZE).  out (1 + D3GA_OBJ_TERMS floats): out[0] = total, out[1..] = color_loss, sil_loss,
 *   scale_loss, fme_loss, blur_loss, vgg_loss, bg_loss (= 0), codes_reg, total_loss.  status (D3GA_OBJ_STATUS_WORDS int32,
 *   zeroed once by the caller): [STEPS] is incremented; on the first call whose total is NaN (not on an infinite one)
 *   [NAN_SEEN] = 1, [FIRST_BAD] = the value of [STEPS] before that call, and words [TERMS .. TERMS + 8] keep that call's terms as
 *   float bits.  One launch of one workgroup.  Calls that share a status cell must be ordered on one stream.
 * d3ga_objective_bwd: every entry with goff >= 0 gets d total / d entry * g[0] written to grads[goff .. goff + len) (n_grads
 *   floats; an entry reaching outside: D3GA_E_SIZE); goff < 0: no gradient.  g on the device.  One launch.
 * ------------------------------------------------------------------------------------------------------- */
#define D3GA_SCALE_ACT_NONE 0
#define D3GA_SCALE_ACT_EXP 1
#define D3GA_SCALE_ENERGY_GRID 1536 /* workgroups of 256 x 4 floats, at most: one pass covers 3 * 2^19 floats */
#define D3GA_OBJ_MAX_FRAMES 16
#define D3GA_OBJ_SLOTS 9
#define D3GA_OBJ_MAX_LEN 4096
#define D3GA_OBJ_TERMS 9
#define D3GA_OBJ_STATUS_NAN_SEEN 0
#define D3GA_OBJ_STATUS_FIRST_BAD 1
#define D3GA_OBJ_STATUS_STEPS 2
#define D3GA_OBJ_STATUS_TERMS 4
#define D3GA_OBJ_STATUS_WORDS 16
typedef struct d3ga_objective_entry {
    const float *ptr;
    int32_t len;
    int32_t goff;
} d3ga_objective_entry;
typedef struct d3ga_objective_desc {
    int32_t n_frames;
    int32_t reserved;
    float lambda_dssim, rgb_weight, sil_weight, fme_weight, blur_weight, vgg_weight;
    d3ga_objective_entry entry[D3GA_OBJ_MAX_FRAMES * D3GA_OBJ_SLOTS]; /* frame-major */
} d3ga_objective_desc;
int d3ga_scale_energy_fwd(int64_t n, const float *scaling, const float *delta, int32_t activation, float *out, float *partials,
                          d3ga_stream_t stream);
int d3ga_scale_energy_bwd(int64_t n, const float *scaling, const float *delta, int32_t activation, const float *g, float *grad,
                          d3ga_stream_t stream);
int d3ga_objective_fwd(const d3ga_objective_desc *desc, float *out, int32_t *status, d3ga_stream_t stream);
int d3ga_objective_bwd(const d3ga_objective_desc *desc, const float *g, float *grads, int64_t n_grads, d3ga_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * The pose prior: the PCA over the refined poses that test.py:264-274 builds once per run, and the clamp of
 * test.py:49-56 that every driven frame goes through.  All arithmetic is float64 (csrc/pose_prior_math.h holds it and its
 * summation orders); poses enter and leave as float32.  No entry point allocates or synchronises; all are capturable; no
 * atomics, every sum in a fixed order that does not depend on the launch geometry: results are reproducible bit for bit.
 *
 * d3ga_pose_fit: table (N,D) float32 -> out (D + D D doubles): the column mean, then the covariance of the centred rows
 *   C = sum_n (x_n - mean)(x_n - mean)^T / (N - 1), row-major and symmetric bit for bit.  Two passes (mean, then covariance) of
 *   two launches each: rows in ascending order inside a chunk of D3GA_POSE_FIT_CHUNK rows, then the chunks in ascending
 *   order.  scratch: d3ga_pose_fit_scratch_bytes(N, D) bytes, 8-byte aligned like out (else D3GA_E_CONFIG).  2 <= N,
 *   1 <= D <= D3GA_POSE_MAX_D, N D <= INT32_MAX (else D3GA_E_SIZE).
 * d3ga_pose_clamp: B >= 1 poses, one workgroup each, in ONE launch.  mean (D), comp (k,D), comp_t (D,k) = its transpose and
 *   std (k) are doubles on the device, 1 <= k <= D3GA_POSE_MAX_D.  stages:
 *     PROJECT | CLIP | RECONSTRUCT   in (B,D) -> out (B,D):   z_j = sum_d (x_d - mean_d) V_jd, d ascending;
 *                                    zc_j = min(max(z_j, -sigma std_j), sigma std_j) (a NaN stays one);
 *                                    out_d = float32((sum_j zc_j V_jd) + mean_d), j ascending
 *     PROJECT                        in (B,D) -> out (B,k) = float32(z)
 *     RECONSTRUCT                    in (B,k) = z -> out (B,D)
 *   (any other combination: D3GA_E_CONFIG).  rows == NULL: pose b is row b of `in`.  rows (B int32 ON THE DEVICE; needs
 *   PROJECT, else D3GA_E_CONFIG): pose b is row rows[b] of the table `in` (n_rows, D); a row outside [0, n_rows) leaves output
 *   row b untouched and sets flag[0] = 1 (sticky: nobody clears it but the caller).  flag must not be NULL with rows.
 * ------------------------------------------------------------------------------------------------------- */
#define D3GA_POSE_MAX_D 256
#define D3GA_POSE_FIT_CHUNK 256
#define D3GA_POSE_STAGE_PROJECT 1
#define D3GA_POSE_STAGE_CLIP 2
#define D3GA_POSE_STAGE_RECONSTRUCT 4
int d3ga_pose_fit_scratch_bytes(int32_t N, int32_t D, int64_t *bytes);
int d3ga_pose_fit(const float *table, int32_t N, int32_t D, double *out, void *scratch, d3ga_stream_t stream);
int d3ga_pose_clamp(const float *in, const int32_t *rows, int32_t n_rows, int32_t B, int32_t D, int32_t k, const double *mean,
                    const double *comp, const double *comp_t, const double *std, double sigma, int32_t stages, float *out,
                    int32_t *flag, d3ga_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * The recorder's frame grid: utils/text_helpers.py:27-50 write_text, the th.cat rows and grid of
 * test.py:145-169 / train.py:344-364, the even-size padding of test.py:176-179 and the uint8 conversions of
 * torchvision.utils.save_image (test.py:182-195) and of train.py:365, as ONE launch that writes every output element exactly
 * once.  No entry point allocates or synchronises; d3ga_frame_grid is capturable; no LDS, no atomics.  The arithmetic is
 * float32, written down in csrc/frame_grid_math.h; the label font is csrc/frame_grid_font.h.
 *
 * desc (HOST, copied into the launch: the panel table and the label bytes travel in the kernel arguments): a canvas
 *   (out_H, out_W), 1..D3GA_GRID_MAX_SIDE each, and 1 <= n_panels <= D3GA_GRID_MAX_PANELS panels.  Panel: src float32 with
 *   ELEMENT strides (sc, sh, sw) >= 0 of channel, row and column, C in {1, 3, 4} source channels (1 is replicated to RGB; a
 *   missing alpha is 1), size (h, w) >= 1 at (y0, x0) inside the canvas; two panels that share a pixel: D3GA_E_CONFIG.  Canvas
 *   pixels that no panel covers get pad_value in every channel.
 * label: label_len <= D3GA_GRID_MAX_LABEL bytes (0: none), drawn in `color` (RGB) from x = X pixels, its baseline
 *   int(10 u) below the panel's top or, with D3GA_PANEL_BOTTOM, int(5 u) above its bottom, u = min(w / 150, 17.7) the unit (25
 *   cells of 6 u fit in the panel's width); D3GA_PANEL_BOLD unites the glyphs with themselves half a unit to the right.  Bytes
 *   outside 32..126 draw as '?'.  Text never leaves its panel and never touches the alpha channel.  One "{:.3f}" in the label
 *   is replaced by value[0] (a float32 ON THE DEVICE, read by the launch) as Python formats it; two of them, or one without
 *   value, or value without one: D3GA_E_CONFIG.
 * mode: D3GA_GRID_OUT_F32_CHW (channels, out_H, out_W) | D3GA_GRID_OUT_F32_HWC (out_H, out_W, channels), dense float32,
 *   unquantised; D3GA_GRID_OUT_U8_SAVE_IMAGE | D3GA_GRID_OUT_U8_CLIP: uint8 (out_H, out_W, channels) with rows `pitch`
 *   bytes apart (>= out_W * channels), quantised as uint8(clamp(x * 255 + 0.5, 0, 255)) (two float32 roundings) |
 *   uint8(clamp(x * 255, 0, 255)); a NaN gives 0.  channels 3 | 4.  flags: D3GA_GRID_BGR writes the colour channels in the
 *   order B, G, R; D3GA_GRID_FORCE_SCALAR takes the one-pixel-per-thread path whatever the alignment.
 * path (HOST, may be NULL): 1 if the launch handles four adjacent pixels per thread with 16-byte loads (out_W, every x0 and
 *   w multiples of 4, every sw = 1, src 16-byte aligned with sc and sh multiples of 4, out 16-byte aligned (uint8: 4-byte
 *   aligned with pitch a multiple of 4)), else 0.  Both paths give the same bytes.
 * d3ga_frame_grid_check: the same tests and the same `path`, no launch (out is not read and may be any non-NULL address).
 * ------------------------------------------------------------------------------------------------------- */
#define D3GA_GRID_MAX_PANELS 16
#define D3GA_GRID_MAX_LABEL 64
#define D3GA_GRID_MAX_SIDE 32768
#define D3GA_GRID_OUT_F32_CHW 0
#define D3GA_GRID_OUT_F32_HWC 1
#define D3GA_GRID_OUT_U8_SAVE_IMAGE 2
#define D3GA_GRID_OUT_U8_CLIP 3
#define D3GA_GRID_BGR 1
#define D3GA_GRID_FORCE_SCALAR 2
#define D3GA_PANEL_BOTTOM 1
#define D3GA_PANEL_BOLD 2
typedef struct d3ga_grid_panel {
    const float *src;
    const float *value; /* NULL unless the label has a "{:.3f}" */
    int64_t sc, sh, sw;
    int32_t C, h, w, y0, x0;
    int32_t flags; /* D3GA_PANEL_* */
    int32_t label_len;
    int32_t X;
    float color[3];
    char label[D3GA_GRID_MAX_LABEL];
} d3ga_grid_panel;
typedef struct d3ga_grid_desc {
    int32_t n_panels, out_H, out_W;
    int32_t mode, channels, flags; /* D3GA_GRID_OUT_*, 3 | 4, D3GA_GRID_* */
    float pad_value;
    int32_t reserved;
    int64_t pitch; /* bytes per output row of the uint8 modes */
    d3ga_grid_panel panel[D3GA_GRID_MAX_PANELS];
} d3ga_grid_desc;
int d3ga_frame_grid_check(const d3ga_grid_desc *desc, const void *out, int32_t *path);
int d3ga_frame_grid(const d3ga_grid_desc *desc, void *out, int32_t *path, d3ga_stream_t stream);

/* ---- PNG files of the written images (csrc/png.hip, csrc/png_math.h) --------------------------------------------
 * A uint8 image (H, W, C), C in {1, 3, 4}, pixels dense and rows `pitch` >= W C bytes apart, becomes the bytes of a PNG file
 * (colour type 0 / 2 / 6, depth 8, no interlace, no ancillary chunk) in two launches, without a host synchronisation and without
 * an allocation; capturable.  The stream is pinned byte for byte by csrc/png_math.h: one IDAT chunk per strip of
 * rows_per_strip rows (0: the default, a function of H, W, C), each a byte-aligned deflate segment of run tokens under its
 * own Huffman table or the fixed one, whichever is smaller.
 *   filter: 0..4 forces a PNG filter type, D3GA_PNG_FILTER_ADAPTIVE chooses per row by the smallest sum of absolute values.
 *   out: 8-byte aligned, [uint64 length][PNG bytes]; out_bytes = room behind the length word, at least d3ga_png_capacity.
 *     Every byte below the length is written exactly once, none at or beyond it.
 *   scratch: 16-byte aligned, at least *scratch_bytes of d3ga_png_capacity; contents need not survive between calls.
 * d3ga_png_capacity (host): the most PNG bytes of such an image, and the scratch it needs; < 0: a status.
 * d3ga_png_check (host): the tests of d3ga_png_encode, no launch; no pointer is read.
 *   Status, nothing launched: C outside {1, 3, 4}, an unknown filter or a misaligned out / scratch D3GA_E_CONFIG; H, W < 1,
 *   rows_per_strip < 0, W C > INT32_MAX, a strip of more than INT32_MAX filtered bytes or pitch < W C D3GA_E_SIZE; a NULL
 *   pointer D3GA_E_NULL; out_bytes or scratch_bytes too small D3GA_E_CAPACITY. */
#define D3GA_PNG_FILTER_ADAPTIVE 5
int64_t d3ga_png_capacity(int32_t H, int32_t W, int32_t C, int32_t rows_per_strip, int64_t *scratch_bytes);
int d3ga_png_check(int32_t H, int32_t W, int32_t C, int64_t pitch, int32_t filter, int32_t rows_per_strip, const void *img, const void *out,
                   int64_t out_bytes, const void *scratch, int64_t scratch_bytes);
int d3ga_png_encode(int32_t H, int32_t W, int32_t C, int64_t pitch, int32_t filter, int32_t rows_per_strip, const void *img, void *out,
                    int64_t out_bytes, void *scratch, int64_t scratch_bytes, d3ga_stream_t stream);

/* ---- Sample preparation (csrc/sample_prep.hip, csrc/sample_prep_math.h) ------------------------------------------
 * What a loader worker does in numpy between the decoded files and the tensors of a sample, one launch for B frames, from the
 * uint8 arrays as the decoder delivers them.  No gradient, no scratch, no atomics, no host synchronisation; capturable.
 * A uint8 source is addressed as  base + b frame + y pitch + x step  in BYTES; no base, pitch or frame stride needs any
 * alignment (an interleaved 747-wide row is 2241 bytes), every read is a byte read and no byte outside the pixels named below is
 * touched.  With B == 1 the frame strides are not read.
 * d3ga_sample_prep_actorshq (datasets/actorshq_dataset.py:244-276, get_boundary_mask :201-217), per pixel (y, x), y < H, x < W:
 *   m         mask[y][x]: channel 0 of the matte, a plane (mask_step 1) or the first byte of an interleaved pixel (mask_step 3);
 *   t         0 if m < 128, 1 if m > 128, 128 if m == 128 (the reference's two masked assignments leave that value alone);
 *   er, di    the minimum / maximum of t over the part of the 3 x 3 window around (y, x) that lies inside the image (cv2.erode /
 *             cv2.dilate with a 3 x 3 kernel of ones, default border value, centre anchor; H and W may be smaller than the window);
 *   boundary  uint8(di - er) == 1, or 5 < m < 250;         fg   t == 1;
 *   label     0 without fg; with fg (r, g, b) = seg[y][x] read as BGR, all three taken as 127 when r + g + b == 0, then in this
 *             order, the last match winning: r == 255 -> 1, g == 255 -> 2, b == 255 -> 3, r == 127 -> 4 (a native red of 127 is
 *             gray as well); seg is not read where there is no fg;
 *   image (B,H,W,3) BGR, pitch >= 3 W;  seg (B,Hs,Ws,3) BGR, Hs >= H, Ws >= W, pitch >= 3 Ws, only its top-left H x W is read;
 *   mask (B,H,W), pitch >= (W - 1) mask_step + 1.
 *   image_out (B,3,H,W) RGB planar, uint8, or float32 with image_f32 = 1 (the same integers);  seg_part_out (B,1,H,W) int32 label;
 *   seg_fg_out, boundary_out (B,1,H,W) float32 0 / 1.  Each may be NULL (skipped).
 * d3ga_sample_prep_goliath (datasets/goliath_dataset.py:454-481): image (B,3,H,W) and parts (B,1,H,W) planar uint8, step 1,
 *   image_plane bytes between two channels; oh = H / 2, ow = W / 2 (an odd last row or column is never read); all outputs float32:
 *   image_out (B,3,oh,ow) and seg_part_out (B,1,oh,ow) the mean of the 2 x 2 block, seg_fg_out that of (parts != 0), boundary_out
 *   1 - seg_fg: F.interpolate(x.float(), scale_factor=0.5, mode="bilinear") bit for bit (multiples of 1/4 below 256).  Each output
 *   may be NULL (skipped; without image_out the image is not read).
 * *path (may be NULL): 1 the launch stored four pixels per thread (16-byte stores; W resp. ow a multiple of 4 and a uint8 image_out
 *   4-byte aligned), 0 one pixel per thread.  Both paths give the same bytes.
 *   Status, nothing launched and *path not written: B, H, W, Hs, Ws <= 0 (Goliath: H or W < 2), B > 65535, H W > INT32_MAX, more
 *   than 262140 (output) rows, Hs < H or Ws < W D3GA_E_SIZE; a pitch smaller than its row, with B > 1 a frame stride (Goliath: or
 *   an image_plane) smaller than what it spans, mask_step outside {1, 3}, image_f32 outside {0, 1}, or a float32 / int32 output not
 *   16-byte aligned D3GA_E_CONFIG; an input NULL or every output NULL D3GA_E_NULL.  Sizes are tested first. */
int d3ga_sample_prep_actorshq(int32_t B, int32_t H, int32_t W, int32_t Hs, int32_t Ws, const uint8_t *image, int64_t image_pitch,
                              int64_t image_frame, const uint8_t *seg, int64_t seg_pitch, int64_t seg_frame, const uint8_t *mask,
                              int64_t mask_pitch, int64_t mask_frame, int32_t mask_step, int32_t image_f32, void *image_out,
                              int32_t *seg_part_out, float *seg_fg_out, float *boundary_out, int32_t *path, d3ga_stream_t stream);
int d3ga_sample_prep_goliath(int32_t B, int32_t H, int32_t W, const uint8_t *image, int64_t image_pitch, int64_t image_plane,
                             int64_t image_frame, const uint8_t *parts, int64_t parts_pitch, int64_t parts_frame, float *image_out,
                             float *seg_part_out, float *seg_fg_out, float *boundary_out, int32_t *path, d3ga_stream_t stream);

/* ---- Part-label transfer onto a mesh (csrc/mesh_labels.hip, csrc/mesh_labels_math.h) ------------------------------
 * What lib/segmentation.py::Segmenter.run does between the rasterizer's fragments and face_to_label.npy (Renderer.forward
 * :59-74, majority_vote :112-123, utils/mesh_utils.py::median_filter_mesh) and lib/cage.py::grow_mask_region :131-153.  All
 * integer, forward only, no host synchronisation, capturable; results do not depend on scheduling.
 *   neighbours (F,3) int32, -1 padded: per face the faces across those of its three edges that occur in exactly two faces
 *   (trimesh's face_adjacency rule, built on the host; a pair that shares two edges appears twice).  An entry outside [0, F)
 *   counts as absent.
 * d3ga_label_vote: B views of H x W vote once each for every face they show.  Two launches.
 *   pick       per view and face f: the pixel with the largest y W + x among those with pix_to_face == f (the last in raster
 *              order: what the reference's index-put keeps on the CPU); none: no vote.  pix_to_face (B,H,W) int32, per-mesh
 *              indices as d3ga_mesh_rasterize writes them; values < 0 or >= F are ignored.
 *   labels     the label image, int32 (label_u8 = 0) or uint8 (1): pixel (b, y, x) at byte  labels + b label_frame +
 *              y label_pitch + x elem  -- (B,1,H,W) and (B,H,W) views, row-padded buffers.  With B == 1 label_frame is not read.
 *   hist       (F,L) int32, L <= D3GA_LABELS_MAX: a pick with label l in [0, L) adds 1 to hist[f][l] (column 0: the views that
 *              saw the face as background); any other label adds nothing and sets D3GA_LABEL_STATUS_RANGE in *status (sticky:
 *              the word is only ever or-ed into).  Every view votes on its own -- a departure from the reference at B > 1, where
 *              the labels of a batch's views are ADDED into each other; at B = 1, its default, the results are the same.
 *   cells      (B,F) uint32 scratch, ALL ZERO on entry and all zero again on exit (the second launch writes back what the
 *              first one set): clear it once.
 *   flags      0, or D3GA_LABEL_EVERY_PIXEL: every pixel sends its atomic (without it a pixel whose right neighbour in the same
 *              wavefront shows the same face sends none).  The results are the same; the flag exists for the measurement.
 * d3ga_label_majority: hist (F,L) -> labels (F,): over labels 1 .. L-1 the largest count, ties to the smallest label; all 0 -> 0.
 * d3ga_label_median: out[f] = the median of labels[n] over f's neighbours (f itself not among them): one -> it, two ->
 *   (a + b) / 2 (labels are not negative), three -> the middle one, none -> labels[f] (the reference raises KeyError there).
 *   out must not be labels.
 * d3ga_label_grow: n_rings rounds of  out[j] = mask[j] | any(i qualifies for i in N(j)),  i qualifying when
 *   0 < #{n in N(i): mask[n]} < #N(i) with duplicates counted on both sides; every round reads the previous round's result only.
 *   mask, out (F,) uint8 (non-zero = set; out holds 0 / 1), no byte in common; scratch 2 F bytes, no byte in common with either, read and
 *   written with n_rings >= 2 only (else may be NULL).  n_rings = 0 copies.  One launch per ring, all enqueued by this call.
 *   Status, nothing launched: a size <= 0, L > D3GA_LABELS_MAX, B > 65535, H W >= INT32_MAX, more than
 *   262140 rows, B F or F L or 3 F > INT32_MAX, n_rings outside [0, D3GA_LABEL_RINGS_MAX] D3GA_E_SIZE; label_u8 outside {0, 1}, an
 *   unknown flag, a pitch smaller than its row, with B > 1 a frame stride smaller than what it spans, an int32 pointer (or int32
 *   label pitch / frame stride) that is no multiple of 4, or buffers that must differ and do not D3GA_E_CONFIG; a required pointer
 *   NULL D3GA_E_NULL.  Sizes are tested first. */
#define D3GA_LABELS_MAX 32
#define D3GA_LABEL_RINGS_MAX 4096
#define D3GA_LABEL_EVERY_PIXEL 1
#define D3GA_LABEL_STATUS_RANGE 1
int d3ga_label_vote(int32_t B, int32_t F, int32_t L, int32_t H, int32_t W, const int32_t *pix_to_face, const void *labels, int32_t label_u8,
                    int64_t label_pitch, int64_t label_frame, uint32_t *cells, int32_t *hist, uint32_t *status, int32_t flags,
                    d3ga_stream_t stream);
int d3ga_label_majority(int32_t F, int32_t L, const int32_t *hist, int32_t *labels, d3ga_stream_t stream);
int d3ga_label_median(int32_t F, const int32_t *neighbours, const int32_t *labels, int32_t *out, d3ga_stream_t stream);
int d3ga_label_grow(int32_t F, int32_t n_rings, const int32_t *neighbours, const uint8_t *mask, uint8_t *out, uint8_t *scratch,
                    d3ga_stream_t stream);

/* ---- Gaussian initialisation: area-weighted surface samples (csrc/gauss_init.hip, csrc/gauss_init_math.h) -----------
 * What lib/cage.py::CageBase.sample_initial_points :262-296 does between a mesh and (points, rotations, faces, barys), and the
 * angle-weighted vertex normals behind `mesh.vertex_normals * inflate` :271-272.  float64 arithmetic, ONE rounding to float32 per
 * output element; the face weights are INTEGERS (areas scaled by a power of two and floored), so the prefix sum is exact and the
 * results depend on neither launch geometry nor scheduling.  The random numbers are an input.  No float atomics, no host
 * synchronisation; capturable.  Additive to ABI 112.
 *
 * d3ga_surface_sample: n samples.  Five launches: clear, largest area (uint64 atomicMax over the doubles' bits), weights + scan
 *   per block of 256 faces, scan of the block totals, one thread per sample.
 *   verts (V,3) f64;  faces (F,3) int32;  face_mask (F) bytes or NULL (0: the face is left out);  uniforms (n,3) f64 in [0,1):
 *   column 0 picks the face, columns 1 and 2 the point (a value outside is clamped for the pick).
 *   points (n,3) f32;  rotations (n,4) f32 wxyz (written with 16-byte stores when 16-byte aligned);  out_faces (n,3) int32 the
 *   vertices of the chosen face;  face_id (n) int32 its index in `faces`;  barys (n,3) f32 of the float32 point.
 *   A face of weight 0 -- masked out, degenerate, below 2^-(62 - ceil(log2 F)) of 2^E (max area < 2^E) -- is never chosen.
 *   scratch: d3ga_surface_sample_scratch_bytes(F) bytes, 256-byte aligned; needs no initialisation and is reusable.
 *   status (sticky, OR-ed): D3GA_SAMPLE_STATUS_EMPTY when every weight is 0 (the outputs are then zeros, face_id -1);
 *   D3GA_SAMPLE_STATUS_RANGE when a face names a vertex outside [0, V) (such a face weighs 0 and nothing is read for it).
 *   block: lanes per workgroup of the per-sample launch, 0 (= 256), 64, 128, 256, 512 or 1024; the results do not depend on it.
 * d3ga_vertex_normals_angle: n_v = normalize(sum over v's faces, in list order, of angle_f(v) normalize(e0 x e1)), zero for a
 *   zero sum; normalize = x / max(|x|, 1e-12).  csr_offsets (V+1), csr_faces: the faces of every vertex, ascending.  normals (V,3)
 *   f64 and / or inflated (V,3) f64 = verts + amount normals; either may be NULL, neither may be verts.  One launch.  A list entry
 *   outside [0, F), a face that does not touch its vertex or names one outside [0, V) is skipped and sets D3GA_SAMPLE_STATUS_RANGE.
 *   Status, nothing launched: V, F, n <= 0, F >= D3GA_SAMPLE_MAX_FACES, 3 V or 4 n > INT32_MAX D3GA_E_SIZE; an unknown block, an
 *   amount that is not finite, a pointer not aligned to its element (scratch: 256 bytes) or an output that is verts
 *   D3GA_E_CONFIG; a required pointer NULL D3GA_E_NULL; scratch_bytes too small D3GA_E_CAPACITY.  Sizes are tested first. */
#define D3GA_SAMPLE_MAX_FACES 16777216 /* 2^24 */
#define D3GA_SAMPLE_STATUS_EMPTY 1
#define D3GA_SAMPLE_STATUS_RANGE 2
int d3ga_surface_sample_scratch_bytes(int32_t F, int64_t *bytes);
int d3ga_surface_sample(int32_t V, int32_t F, int32_t n, const double *verts, const int32_t *faces, const uint8_t *face_mask,
                        const double *uniforms, float *points, float *rotations, int32_t *out_faces, int32_t *face_id, float *barys,
                        void *scratch, int64_t scratch_bytes, uint32_t *status, int32_t block, d3ga_stream_t stream);
int d3ga_vertex_normals_angle(int32_t V, int32_t F, const double *verts, const int32_t *faces, const int32_t *csr_offsets,
                              const int32_t *csr_faces, double amount, double *normals, double *inflated, uint32_t *status,
                              d3ga_stream_t stream);

/* ---- Template binding: Loop subdivision with attribute columns, unpose (csrc/template_bind.hip, csrc/template_bind_math.h;
 * DESIGN.md 4.4t) ---------------------------------------------------------------------------------------------------------------
 * What lib/smplman.py::Smplman.create_body_model :67-110 and lib/cage_smplman.py::CageSmpl.create_cage_model :54-76 need between a
 * body model and (skin_weights, nn_ids, body_template_vertices): utils/mesh_utils.py::subdivide_loop :105-325 and Smplman.unpose
 * :55-59.  float64 arithmetic, ONE rounding to float32 per output element, every sum in a fixed order (the header states them); no
 * float atomics; the results depend on neither launch geometry nor scheduling.  No host synchronisation.  Additive to ABI 112.
 *
 * One level of topology is a d3ga_loop_plan.  Unique edges are numbered in ascending order of (larger endpoint, smaller endpoint).
 *   d3ga_loop_edge_keys: keys[3 f + c] = larger << 32 | smaller of face edge c = (faces[f][c], faces[f][(c + 1) % 3]); a face that names
 *     a vertex outside [0, V) (D3GA_BIND_STATUS_RANGE) or one vertex twice (D3GA_BIND_STATUS_DEGENERATE) gets D3GA_LOOP_BAD_KEY three
 *     times and takes no part in the plan.  The caller sorts the keys (stable, ascending) and passes them on with the permutation.
 *   d3ga_loop_plan_build: fills the tables of `plan` (every table sized for E = 3 F; plan->E is not read) from the sorted keys and
 *     `perm` (sorted position -> face edge).  info (4 int32): [0] = E, [1] = the largest valence, [2] = the status word (sticky:
 *     OR-ed, never cleared -- pass it to d3ga_loop_edge_keys as well), [3] unused.  An edge in three or more faces sets D3GA_BIND_STATUS_NONMANIFOLD (its first two faces are kept).  A vertex is a
 *     boundary vertex when it is an end of an edge of one face.  Neighbour lists are ascending.  scratch:
 *     d3ga_loop_plan_scratch_bytes(V, F) bytes, 256-byte aligned, no initialisation needed.
 *   d3ga_loop_subdivide: x (V, D) f64 -> out (V + E, D) f32; rows 0..V-1 the even vertices, row V + e the odd vertex of edge e.
 *     odd, interior: 0.375 x0 + 0.375 x1 + x2 / 8 + x3 / 8 (x0 the smaller endpoint, x2 opposite in the face of lower index), left to
 *     right; odd, boundary: (x0 + x1) / 2; even, interior: beta[k] S + (1 - k beta[k]) x, S the neighbours' sum in ascending index
 *     order; even, boundary: S' / 8 + 0.75 x, S' over the neighbours that are boundary vertices (every one, also across an interior
 *     edge); a vertex of no face: x.  beta (n_beta) f64 on the device, indexed by valence k; n_beta > the largest valence.
 *   d3ga_loop_faces: face f = (a, b, c) -> rows 4f..4f+3 = (a,o0,o2), (o0,b,o1), (o2,o1,c), (o0,o1,o2), o_c = V + face_edge[3 f + c].
 * d3ga_unpose: x_i = M^-1 (v_i - t / s) - offsets[r], r = rows[i] (rows NULL: r = i), [M t; 0 0 0 s] = sum_j w_rj A_j in float64, M^-1
 *   the cofactor inverse.  Terms of weight 0 are skipped, the others are added in stored order.  vertices (n,3) f64; joint_mats
 *   (J,4,4) f64 row-major (the bottom rows are taken as 0 0 0 1); skin_w (R, K) f32 (w_f64 = 0) or f64 (1); skin_idx (R, K) int32, or
 *   NULL for the dense table (K = J); rows (n) int64 or NULL; offsets (n_offsets, 3) f64 or NULL; out (n,3) f32.  |det M| or |s|
 *   below 1e-12 (or not a number) sets D3GA_BIND_STATUS_SINGULAR and the row is zeros; a row or a joint outside its table sets
 *   D3GA_BIND_STATUS_RANGE (the row is zeros, the joint is skipped).  One launch.
 *   Status, nothing launched: V, F, D, n, J, R, K <= 0, 6 F > INT32_MAX, R K or 16 J > INT32_MAX, K != J with the dense table D3GA_E_SIZE; a
 *   required pointer NULL D3GA_E_NULL; a pointer not aligned to its element (scratch: 256 bytes) D3GA_E_CONFIG; scratch_bytes too
 *   small D3GA_E_CAPACITY.  Sizes are tested first. */
#define D3GA_BIND_STATUS_RANGE 1
#define D3GA_BIND_STATUS_NONMANIFOLD 2
#define D3GA_BIND_STATUS_DEGENERATE 4
#define D3GA_BIND_STATUS_SINGULAR 8
#define D3GA_LOOP_BAD_KEY 0x7fffffffffffffffLL
typedef struct d3ga_loop_plan {
    int32_t V, F, E, reserved;
    int32_t *edge_verts;     /* (E,2) smaller, larger endpoint */
    int32_t *edge_opp;       /* (E,2) the opposite vertex in the face of lower index; in the other face, or -1 */
    int32_t *edge_faces;     /* (E,2) the face of lower index; the other face, or -1 */
    uint8_t *edge_boundary;  /* (E) 1: the edge has one face */
    int32_t *face_edge;      /* (3 F) face edge -> unique edge (-1: a face that takes no part) */
    int32_t *vert_offsets;   /* (V + 1) */
    int32_t *vert_nbr;       /* (2 E) the neighbours of every vertex, ascending */
    uint8_t *vert_boundary;  /* (V) */
} d3ga_loop_plan;
int d3ga_loop_edge_keys(int32_t V, int32_t F, const int32_t *faces, int64_t *keys, uint32_t *status, d3ga_stream_t stream);
int d3ga_loop_plan_scratch_bytes(int32_t V, int32_t F, int64_t *bytes);
int d3ga_loop_plan_build(const d3ga_loop_plan *plan, const int32_t *faces, const int64_t *sorted_keys, const int64_t *perm, int32_t *info,
                         void *scratch, int64_t scratch_bytes, d3ga_stream_t stream);
int d3ga_loop_subdivide(const d3ga_loop_plan *plan, int32_t D, const double *x, const double *beta, int32_t n_beta, float *out,
                        uint32_t *status, d3ga_stream_t stream);
int d3ga_loop_faces(const d3ga_loop_plan *plan, const int32_t *faces, int32_t *out, d3ga_stream_t stream);
int d3ga_unpose(int32_t n, int32_t J, int32_t R, int32_t K, const double *vertices, const double *joint_mats, const void *skin_w,
                int32_t w_f64, const int32_t *skin_idx, const int64_t *rows, const double *offsets, int32_t n_offsets, float *out,
                uint32_t *status, d3ga_stream_t stream);

/* ---- Cage surface authoring: voxelise, fill, isosurface, smooth, parts (csrc/cage_author.hip, csrc/cage_author_math.h; DESIGN.md
 * 4.4u) ----------------------------------------------------------------------------------------------------------------------------
 * What cager/ops.py::cage_processor :140-148 does between the star-pose body mesh and the surface TetGen fills, without trimesh,
 * mcubes or open3d; parity with those packages is UNPINNED -- the rules are the header's.  float64 arithmetic, one rounding to
 * float32 per output element, fixed summation orders, integer atomics only; results depend on neither launch geometry nor
 * scheduling.  No kernel waits on another workgroup: where a step must see the whole grid the launch boundary is the hand-off.
 * No entry point synchronises with the host; the caller reads `changed` / `counts` back between calls.  Additive to ABI 112.
 *
 * A d3ga_voxel_grid is D = 2 radius + 1 voxels per axis, bit-packed along x: word ((z D + y) W + (x >> 6)), bit x & 63,
 * W = ceil(D / 64); voxel (i,j,k) is the closed cube of side pitch = 1 / (radius + 0.1) centred at ((i,j,k) - radius) pitch.
 *   d3ga_cage_voxelize: clears the grid, then sets every voxel some triangle meets (13-axis separating-axis test, float64, the
 *     header's operation order; integer atomicOr).  verts (V,3) f64, faces (F,3) int32.  Geometry outside the grid is clipped.  A face
 *     index outside [0, V) or a coordinate that is not finite sets D3GA_CAGE_STATUS_RANGE and the face is left out.
 *   d3ga_cage_fill: scipy.ndimage.binary_fill_holes in stages.  BEGIN: outside = the empty border voxels.  ROUND: one sweep along
 *     x, y and z, forward and back; *changed |= 1 if a bit was set (the caller clears it, reads it back and repeats ROUND until it
 *     stays 0).  FINISH: filled = everything but outside.  `outside` and `filled` are grids' bit arrays of the same size as surface->bits.
 *   d3ga_cage_iso_count / _emit: marching tetrahedra (six Kuhn tetrahedra per cell, the grid padded with one empty layer).  count
 *     leaves the prefix sums in scratch (d3ga_cage_iso_scratch_bytes(radius), 256-byte aligned) and counts[0] = vertices,
 *     counts[1] = faces (device int64); emit, with the same scratch, writes vertices (n_vertices,3) f32 =
 *     ((x / radius - 1) + centre) / scale per coordinate and faces (n_faces,3) int32, oriented from occupied to empty.
 *   d3ga_cage_smooth: `iterations` Jacobi iterations on x (V,3) f64 (overwritten; work and normals are (V,3) f64 scratch), neighbours
 *     from plan->vert_offsets / vert_nbr; out (V,3) f32.  IMPROVED: the normal-aware Laplacian with step lam (mu unused); needs faces
 *     and the vertex -> face lists csr_offsets (V+1) / csr_faces (ascending).  TAUBIN: two uniform steps per iteration, lam then mu.
 *     Status bits: D3GA_CAGE_STATUS_ISOLATED (a vertex of no face or no neighbour), _ZERO_EDGE (a neighbour at distance 0); such a
 *     vertex stays where it is.
 *   d3ga_cage_components: BEGIN: label[f] = f.  ROUND: every edge of plan->edge_faces hooks the larger of its two roots to the
 *     smaller (integer atomicMin), then every face jumps to its root; *changed |= 1 if an edge joined two roots.  At the fixed
 *     point label[f] is the smallest face index of f's part.
 *   Status, nothing launched: radius outside 1 .. D3GA_CAGE_MAX_RADIUS or D, W that do not belong to it, sizes <= 0 or past
 *   INT32_MAX / 3, iterations outside 1 .. D3GA_CAGE_MAX_ITERATIONS D3GA_E_SIZE; a required pointer NULL D3GA_E_NULL; a pointer not
 *   aligned to its element (scratch: 256 bytes), an unknown stage or mode, aliased buffers, values that are not finite D3GA_E_CONFIG;
 *   scratch_bytes too small D3GA_E_CAPACITY. */
#define D3GA_CAGE_MAX_RADIUS 511
#define D3GA_CAGE_MAX_ITERATIONS 4096
#define D3GA_CAGE_STATUS_RANGE 1
#define D3GA_CAGE_STATUS_ISOLATED 2
#define D3GA_CAGE_STATUS_ZERO_EDGE 4
#define D3GA_CAGE_FILL_BEGIN 0
#define D3GA_CAGE_FILL_ROUND 1
#define D3GA_CAGE_FILL_FINISH 2
#define D3GA_CAGE_SMOOTH_IMPROVED 0
#define D3GA_CAGE_SMOOTH_TAUBIN 1
#define D3GA_CAGE_PARTS_BEGIN 0
#define D3GA_CAGE_PARTS_ROUND 1
typedef struct d3ga_voxel_grid {
    int32_t radius, D, W, reserved;
    uint64_t *bits;          /* (D, D, W) words indexed [z][y][x >> 6] */
} d3ga_voxel_grid;
typedef struct d3ga_cage_iso_desc {
    int32_t n_vertices, n_faces;     /* what d3ga_cage_iso_count reported */
    double centre[3], scale[3];
    float *vertices;         /* (n_vertices, 3) */
    int32_t *faces;          /* (n_faces, 3) */
} d3ga_cage_iso_desc;
typedef struct d3ga_cage_smooth_desc {
    int32_t mode, iterations;
    double lam, mu;
    double *x, *work, *normals;      /* (V,3) each; normals may be NULL for TAUBIN */
    const int32_t *faces, *csr_offsets, *csr_faces;      /* IMPROVED only */
    float *out;              /* (V,3) */
    uint32_t *status;
} d3ga_cage_smooth_desc;
int d3ga_cage_voxelize(const d3ga_voxel_grid *grid, int32_t V, int32_t F, const double *verts, const int32_t *faces, uint32_t *status,
                       d3ga_stream_t stream);
int d3ga_cage_fill(const d3ga_voxel_grid *surface, int32_t stage, uint64_t *outside, uint64_t *filled, int32_t *changed, d3ga_stream_t stream);
int d3ga_cage_iso_scratch_bytes(int32_t radius, int64_t *bytes);
int d3ga_cage_iso_count(const d3ga_voxel_grid *grid, void *scratch, int64_t scratch_bytes, int64_t *counts, d3ga_stream_t stream);
int d3ga_cage_iso_emit(const d3ga_voxel_grid *grid, const d3ga_cage_iso_desc *out, void *scratch, int64_t scratch_bytes, d3ga_stream_t stream);
int d3ga_cage_smooth(const d3ga_loop_plan *plan, const d3ga_cage_smooth_desc *smooth, d3ga_stream_t stream);
int d3ga_cage_components(const d3ga_loop_plan *plan, int32_t stage, int32_t *label, int32_t *changed, d3ga_stream_t stream);

/* ---- Quadric edge-collapse decimation of the cage surface (csrc/decimate.hip, csrc/decimate_math.h) -----------------
 * What cager/ops.py::simplify :121-137 asks of open3d's simplify_quadric_decimation, as ROUNDS OF INDEPENDENT COLLAPSES; parity with
 * open3d's serial queue is UNPINNED -- the rules are the header's.  float64 arithmetic in a fixed order, integer atomics only; the
 * result depends on the mesh and the target alone.  No kernel waits on another workgroup and no entry point synchronises with the
 * host: per round the caller builds the d3ga_loop_plan of the current faces and their vertex -> face lists, calls the stages in
 * order, sorts `keys` (ascending, signed 64-bit) between candidates and collapse, and reads `counts` back after faces.  Additive to
 * ABI 112.
 *   d3ga_decimate_quadrics (once): quadrics[v] = the sum of area * p p^T over the faces of v in ascending face index, p the unit
 *     plane of the face, as 10 float64 (xx xy xz xw yy yz yw zz zw ww).  A face without area adds nothing.
 *   d3ga_decimate_candidates: owner[v] = all ones, remap[v] = v, counts[1] = 0; then for every edge e = (u, w), u < w, of the plan:
 *     keys[e] = (float32 bits of the cost) << 32 | e and placement[e] = the point both ends move to, or keys[e] = D3GA_LOOP_BAD_KEY
 *     for an edge that must not collapse (a boundary end, the link condition, a flipped face, a cost that is not finite).
 *     counts[1] += the number of valid edges.
 *   d3ga_decimate_collapse: the first n_admit entries of sorted_keys that are valid are admitted.  Launch 1: each does a 64-bit
 *     integer atomicMin of its key into owner[u] and owner[w].  Launch 2: an admitted edge with owner[t] >= key for every t in the
 *     closed neighbourhoods of u and w is selected and applied: x[u] = placement[e], quadrics[u] += quadrics[w], remap[w] = u.
 *   d3ga_decimate_faces: every face is relabelled through remap; the faces that still name three vertices are written to faces_out
 *     in order; counts[0] = their number.  scratch: d3ga_decimate_scratch_bytes(F) bytes, 256-byte aligned, no initialisation needed.
 *   A table entry outside its table sets D3GA_CAGE_STATUS_RANGE in *status (sticky) and is left out.  D3GA_CAGE_STATUS_STUCK is set
 *   by the caller when a round finds no valid edge or the round limit is reached.
 *   Status, nothing launched: sizes as d3ga_cage_smooth; n_admit outside 1 .. E D3GA_E_SIZE; a required pointer NULL D3GA_E_NULL; a
 *   pointer not aligned to its element (scratch: 256 bytes) or faces_out == faces D3GA_E_CONFIG; scratch too small D3GA_E_CAPACITY. */
#define D3GA_CAGE_STATUS_STUCK 8
typedef struct d3ga_decimate_desc {
    int32_t n_admit, reserved;       /* collapse: how many of the cheapest edges are admitted */
    double *x;                       /* (V,3) positions */
    double *quadrics;                /* (V,10) */
    const int32_t *faces;            /* (F,3) the faces the plan was built from */
    const int32_t *csr_offsets, *csr_faces;      /* vertex -> faces, ascending: (V+1), (3 F) */
    int64_t *keys;                   /* (E) candidates writes them */
    double *placement;               /* (E,3) */
    const int64_t *sorted_keys;      /* (E) collapse reads them */
    uint64_t *owner;                 /* (V) */
    int32_t *remap;                  /* (V) */
    int32_t *faces_out;              /* (F,3) */
    void *scratch;
    int64_t scratch_bytes;
    int64_t *counts;                 /* [0] faces after the round, [1] valid edges of the round */
    uint32_t *status;
} d3ga_decimate_desc;
int d3ga_decimate_scratch_bytes(int32_t F, int64_t *bytes);
int d3ga_decimate_quadrics(const d3ga_loop_plan *plan, const d3ga_decimate_desc *desc, d3ga_stream_t stream);
int d3ga_decimate_candidates(const d3ga_loop_plan *plan, const d3ga_decimate_desc *desc, d3ga_stream_t stream);
int d3ga_decimate_collapse(const d3ga_loop_plan *plan, const d3ga_decimate_desc *desc, d3ga_stream_t stream);
int d3ga_decimate_faces(const d3ga_loop_plan *plan, const d3ga_decimate_desc *desc, d3ga_stream_t stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* D3GA_H */
