"""The Goliath body model: `lbsmodel.body_model.LBSModule` / `LinearBlendSkinning` / `ParameterTransform` as the reference
builds and calls them (lib/blueman.py:27-56, 101-168; lib/cage_blueman.py:85-89), with the skeleton solved by the HIP kernels
of csrc/skeleton.hip (include/d3ga.h, B2) and the skinning done by `cage_deform.lbs_cage`.  Constructor signatures, attribute
names and buffer names are the reference's, so a reference checkpoint's `lbs_module.*` entries load with strict=True.

Conventions (restated; tests/goliath_ref.py is the float64 oracle, tests/golden/skeleton_cases.npz the reference's own values):
  state       (B,J,8) = translation 3 | quaternion xyzw 4 | scale 1.  Quaternions are used AS GIVEN: nothing is normalised, and
              the inverse of the bind rotation divides by |q|^2.  (`cage_deform.skeleton_matrices` normalises first and is a
              different function.)
  parameters  every joint has 7 skeleton parameters [t 3 | Euler xyz 3 | log2 scale] = transform . [poses; scales] +
              transform_offsets, `transform` (7J, n_pose + n_scale) sparse in practice (kept as CSR / CSC, nonzeros only).
  local       translation t + joint_offset; rotation joint_rotation (x) q(Euler), q built from the half angles
              (-rx/2, ry/2, rz/2); scale 2^p.
  chain       q = q_p (x) q_l, t = rot(q_p, t_l s_p) + t_p, s = s_p s_l; a joint with parent -1 is a root.  Parents must
              precede their children (ValueError naming the joint otherwise).
  matrices    (B,J,3,4) = [R(q_t (x) q_b^-1) s_t / s_b | t] against bind_state, the state of the all-zero parameter vector.
  root        the matrix of joint 1 (`ROOT_JOINT`, fixed in the reference) of the solve with ZERO scales.

`skin_weights`, `skin_indices`, `lbs_template_verts`, `bind_state` and every skeleton buffer are read when a call is made:
the reference reassigns them after construction (lib/cage_blueman.py:85-89).  Device tables derived from them are cached by
the storage (address, version) of their sources.  Buffers must stay float32 on the GPU: a `.double()` / `.half()` module is
refused (TypeError) and CPU tensors are refused (D3GAError) before anything is launched; inputs may be of any float dtype.

`compute_relative_rigid_transforms`, `unpose`, `unskinning` and `compute_joints_weights` run once at set-up
(Blueman.to_body_model_space) and are plain torch on whatever device the module lives."""
import ctypes
import weakref

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._lib import check, dptr, require_cuda, stream_handle
from .body_model import tree_tables
from .cage_deform import StorageCache, _i32c, lbs_cage

ROOT_JOINT = 1


# ----------------------------------------------------------------------------------------------------------------------
# plain torch forms (set-up paths, bind state at construction, the eager baseline of tools/time_skeleton.py)
# ----------------------------------------------------------------------------------------------------------------------
def _qmul(a, b):
    ax, ay, az, aw = a.unbind(-1)
    bx, by, bz, bw = b.unbind(-1)
    return torch.stack([ax * bw + ay * bz - az * by + aw * bx, -ax * bz + ay * bw + az * bx + aw * by,
                        ax * by - ay * bx + az * bw + aw * bz, -ax * bx - ay * by - az * bz + aw * bw], -1)


def _qrot(q, v):
    shape = torch.broadcast_shapes(q[..., :3].shape, v.shape)
    a, v = q[..., :3].expand(shape), v.expand(shape)
    av = torch.cross(a, v, dim=-1)
    return v + 2.0 * (av * q[..., 3:] + torch.cross(a, av, dim=-1))


def _qinv(q):
    return q * q.new_tensor([-1.0, -1.0, -1.0, 1.0]) / (q * q).sum(-1, keepdim=True)


def _euler_quat(r):
    h = r * r.new_tensor([-0.5, 0.5, 0.5])
    c, s = torch.cos(h), torch.sin(h)
    c0, c1, c2, s0, s1, s2 = c[..., 0], c[..., 1], c[..., 2], s[..., 0], s[..., 1], s[..., 2]
    return torch.stack([-s0 * (c1 * c2) - c0 * (s1 * s2), c0 * (s1 * c2) - s0 * (c1 * s2), c0 * (c1 * s2) + s0 * (s1 * c2),
                        c0 * (c1 * c2) - s0 * (s1 * s2)], -1)


def _local_torch(param, joint_offset, joint_rotation):
    p = param.reshape(param.shape[0], -1, 7)
    return p[..., 0:3] + joint_offset, _qmul(joint_rotation[None], _euler_quat(p[..., 3:6])), torch.exp2(p[..., 6:7])


def _compose(outer, inner):
    """The similarity `outer . inner` of two states (..., 8): rotations multiply, scales multiply, inner's translation goes
    through outer's scale and rotation.  A child's state is _compose(parent, local); a joint's map against the bind pose is
    _compose(target, inverse bind)."""
    oq, os_ = outer[..., 3:7], outer[..., 7:8]
    return torch.cat([_qrot(oq, inner[..., 0:3] * os_) + outer[..., 0:3], _qmul(oq, inner[..., 3:7]), os_ * inner[..., 7:8]], -1)


def _invert_state(state):
    """The state of the inverse similarity (quaternion inverse through |q|^2, no normalisation)."""
    qi, si = _qinv(state[..., 3:7]), 1.0 / state[..., 7:8]
    return torch.cat([_qrot(qi, -state[..., 0:3]) * si, qi, si], -1)


def _quat_columns(q):
    """(..., 3, 3) whose column c is e_c pushed through _qrot(q, .): the rotation matrix when |q| = 1."""
    eye = torch.eye(3, dtype=q.dtype, device=q.device)
    return torch.stack([_qrot(q, eye[c].expand(q.shape[:-1] + (3,))) for c in range(3)], -1)


def solve_skeleton_state_torch(param, joint_offset, joint_rotation, joint_parents):
    """The skeleton solve as eager torch ops, one joint after the other (any device, any float dtype)."""
    local = torch.cat(_local_torch(param, joint_offset, joint_rotation), -1)
    out = []
    for j, p in enumerate(joint_parents.reshape(-1).tolist()):
        out.append(local[:, j] if p < 0 else _compose(out[p], local[:, j]))
    return torch.stack(out, 1)


def _relative_states(bind_state, target_states):
    """(B,J,8): every joint's map from the bind pose to the target pose, as a state."""
    return _compose(target_states, _invert_state(bind_state.reshape(1, -1, 8)).expand_as(target_states))


def states_to_matrix_torch(bind_state, target_states):
    """(B,J,3,4) joint matrices as eager torch ops (any device, any float dtype)."""
    rel = _relative_states(bind_state, target_states)
    return torch.cat([_quat_columns(rel[..., 3:7]) * rel[..., 7:8, None], rel[..., 0:3, None]], -1)


# ----------------------------------------------------------------------------------------------------------------------
# kernel tables
# ----------------------------------------------------------------------------------------------------------------------
def check_parents(parents):
    """parents (J,) as a list of ints, validated: -1 marks a root, every other parent is an EARLIER joint."""
    par = [int(p) for p in np.asarray(parents).reshape(-1)]
    J = len(par)
    if not 2 <= J <= _lib.SKEL_MAX_JOINTS:
        raise ValueError(f"{J} joints: the skeleton kernels take 2 to {_lib.SKEL_MAX_JOINTS}")
    for j, p in enumerate(par):
        if p == j:
            raise ValueError(f"joint {j} is its own parent")
        if p < -1 or p >= J:
            raise ValueError(f"joint {j} has parent {p}, outside [-1, {J})")
        if p > j:
            raise ValueError(f"joint {j} comes before its parent {p}: parents must precede their children")
    return par


def transform_tables(transform):
    """CSR and CSC of a dense (R, P) parameter transform, nonzeros only, float64 in -> dict of numpy arrays:
    csr_ptr (R+1), csr_col (columns ascending within a row), csr_val; csc_ptr (P+1), csc_row (rows ascending within a column),
    csc_val.  Empty rows and columns are empty ranges."""
    T = np.asarray(transform)
    R, P = T.shape
    rows, cols = np.nonzero(T)                               # row-major: by row, columns ascending
    csr_ptr = np.searchsorted(rows, np.arange(R + 1)).astype(np.int32)
    order = np.lexsort((rows, cols))                         # by column, rows ascending
    csc_ptr = np.searchsorted(cols[order], np.arange(P + 1)).astype(np.int32)
    return dict(csr_ptr=csr_ptr, csr_col=cols.astype(np.int32), csr_val=T[rows, cols],
                csc_ptr=csc_ptr, csc_row=rows[order].astype(np.int32), csc_val=T[rows[order], cols[order]])


def csr_apply(tab, x):
    """transform . x through the CSR (numpy, the dtype of the tables): the kernel's sum, in its order."""
    out = np.zeros(len(tab["csr_ptr"]) - 1, dtype=tab["csr_val"].dtype)
    for r in range(len(out)):
        for k in range(tab["csr_ptr"][r], tab["csr_ptr"][r + 1]):
            out[r] += tab["csr_val"][k] * x[tab["csr_col"][k]]
    return out


def csc_apply_t(tab, g):
    """transform^T . g through the CSC (numpy)."""
    out = np.zeros(len(tab["csc_ptr"]) - 1, dtype=tab["csc_val"].dtype)
    for p in range(len(out)):
        for k in range(tab["csc_ptr"][p], tab["csc_ptr"][p + 1]):
            out[p] += tab["csc_val"][k] * g[tab["csc_row"][k]]
    return out


_plan_cache = {}
_PLAN_FLOATS = ("joint_offset", "joint_rotation", "transform_offsets", "csr_val", "csc_val")
_PLAN_INTS = ("parents", "level_ptr", "level_joint", "child_ptr", "child_joint", "csr_ptr", "csr_col", "csc_ptr", "csc_row")


def _require_f32(what, **tensors):
    bad = [f"{k} {t.dtype}" for k, t in tensors.items() if t is not None and t.dtype != torch.float32]
    if bad:
        raise TypeError(f"{what}: the kernels read float32 buffers, these are not: {', '.join(bad)}.  Keep the module in "
                        "float32 (no .double() / .half()); the inputs may be of any float dtype.")


def skeleton_plan(joint_parents, joint_offset, joint_rotation, transform=None, transform_offsets=None):
    """The device tables of a skeleton (struct d3ga_skeleton), built once per set of source tensors and cached by their
    storage (address, version): tree levels, children CSR, the parameter transform as CSR + CSC.  transform=None: the plan of
    the free function `solve_skeleton_state`, which takes the 7J skeleton parameters as they are.  Building reads the tables
    back to the host once; calls that hit the cache neither synchronise nor allocate.  A plan lives exactly as long as its
    source tensors (weak references): nothing is evicted by count, so the table addresses a captured graph has recorded stay
    valid while the module that owns the sources is alive, and a plan whose sources are gone is dropped on the next miss."""
    srcs = (joint_parents, joint_offset, joint_rotation, transform, transform_offsets)
    key = tuple((t.data_ptr(), t._version, tuple(t.shape), t.dtype, t.device) if t is not None else None for t in srcs)
    hit = _plan_cache.get(key)
    if hit is not None and all(r() is not None for r in hit["refs"]):
        return hit
    for k in [k for k, v in _plan_cache.items() if any(r() is None for r in v["refs"])]:
        del _plan_cache[k]                  # a source died: its address may be recycled, and nothing can call with it again
    _require_f32("skeleton", joint_offset=joint_offset, joint_rotation=joint_rotation, transform=transform,
                 transform_offsets=transform_offsets)
    par = check_parents(joint_parents.detach().cpu().numpy())
    require_cuda(joint_parents, joint_offset, joint_rotation, transform, transform_offsets)
    J = len(par)
    if tuple(joint_offset.shape) != (J, 3) or tuple(joint_rotation.shape) != (J, 4):
        raise ValueError(f"joint_offset must be ({J},3) and joint_rotation ({J},4), got {tuple(joint_offset.shape)} and "
                         f"{tuple(joint_rotation.shape)}")
    dev = joint_offset.device
    if transform is not None:
        if transform.dim() != 2 or transform.shape[0] != 7 * J or transform_offsets.numel() != 7 * J:
            raise ValueError(f"transform must be ({7 * J}, n_params) and transform_offsets hold {7 * J} values, got "
                             f"{tuple(transform.shape)} and {tuple(transform_offsets.shape)}")
        tab = transform_tables(transform.detach().cpu().numpy())
        n_params = transform.shape[1]
        offs = transform_offsets.detach().reshape(-1).contiguous()
    else:
        tab = transform_tables(np.zeros((7 * J, 0), dtype=np.float32))
        n_params = 0
        offs = torch.zeros(7 * J, dtype=torch.float32, device=dev)
    # the tree tables handle one root at index 0 or several: roots are the joints with parent -1
    level_ptr, level_joint, child_ptr, child_joint, _ = tree_tables(np.asarray(par, dtype=np.int64))
    arrays = dict(parents=np.asarray(par, dtype=np.int32), level_ptr=level_ptr, level_joint=level_joint, child_ptr=child_ptr,
                  child_joint=child_joint, **tab)
    plan = dict(J=J, n_params=n_params, n_levels=len(level_ptr) - 1, n_children=len(child_joint),
                refs=[weakref.ref(t) for t in srcs if t is not None],
                joint_offset=joint_offset.detach().contiguous(), joint_rotation=joint_rotation.detach().contiguous(),
                transform_offsets=offs)
    for k in _PLAN_INTS + ("csr_val", "csc_val"):
        a = np.ascontiguousarray(arrays[k], dtype=np.float32 if k.endswith("val") else np.int32)
        if a.size == 0:                     # an empty tensor's device pointer is NULL, which the C ABI refuses; never read
            a = np.zeros(1, a.dtype)
        plan[k] = torch.from_numpy(a).to(dev)
    s = _lib.Skeleton(J=J, n_params=n_params, n_levels=plan["n_levels"], n_children=plan["n_children"])
    for k in _PLAN_INTS + _PLAN_FLOATS:
        setattr(s, k, plan[k].data_ptr())
    plan["struct"] = s
    _plan_cache[key] = plan
    return plan


class _SkeletonFn(torch.autograd.Function):
    """One skeleton launch: states, matrices and root transforms of `n_sets` scale sets (set 0: `scales`, the rest: zeros)."""

    @staticmethod
    def forward(ctx, plan, bind, poses, scales, direct, n_sets, want_mats, want_root, trans_scale):
        require_cuda(bind, poses, scales, direct)
        src = direct if direct is not None else poses
        B, dev, J = src.shape[0], src.device, plan["J"]
        pw = 0 if direct is not None else poses.shape[1]
        states = torch.empty((n_sets, B, J, 8), dtype=torch.float32, device=dev)
        saved = torch.empty((n_sets, B, J, _lib.SKEL_SAVED_FLOATS), dtype=torch.float32, device=dev)
        mats = torch.empty((n_sets, B, J, 4, 4), dtype=torch.float32, device=dev) if want_mats else None
        root = torch.empty((n_sets, B, 12), dtype=torch.float32, device=dev) if want_root else None
        check(_lib.lib().d3ga_skeleton_fwd(ctypes.byref(plan["struct"]), B, n_sets, pw, dptr(poses), dptr(scales),
                                           1 if scales is None else scales.shape[0], dptr(direct), dptr(bind), trans_scale,
                                           ROOT_JOINT, dptr(states), dptr(saved), dptr(mats), dptr(root), stream_handle()),
              "d3ga_skeleton_fwd")
        ctx.plan, ctx.n_sets, ctx.pw, ctx.direct, ctx.trans_scale = plan, n_sets, pw, direct is not None, trans_scale
        ctx.scale_rows = None if scales is None else scales.shape[0]
        ctx.save_for_backward(states, saved, bind if bind is not None else torch.empty(0, device=dev))
        ctx.has_bind = bind is not None
        ctx.set_materialize_grads(False)
        return states, mats, root

    @staticmethod
    def backward(ctx, g_states, g_mats, g_root):
        states, saved, bind = ctx.saved_tensors
        plan, need = ctx.plan, ctx.needs_input_grad
        n_sets, B, J = states.shape[0], states.shape[1], plan["J"]
        dev = states.device
        g_states, g_mats, g_root = (None if g is None else g.float().contiguous() for g in (g_states, g_mats, g_root))
        ns = plan["n_params"] - ctx.pw
        gp = torch.empty((B, ctx.pw), dtype=torch.float32, device=dev) if (need[2] and not ctx.direct) else None
        gs = torch.empty((B, ns), dtype=torch.float32, device=dev) if (need[3] and ctx.scale_rows is not None) else None
        gd = torch.empty((B, 7 * J), dtype=torch.float32, device=dev) if (need[4] and ctx.direct) else None
        check(_lib.lib().d3ga_skeleton_bwd(ctypes.byref(plan["struct"]), B, n_sets, ctx.pw, int(ctx.direct),
                                           dptr(bind if ctx.has_bind else None), ctx.trans_scale, ROOT_JOINT, dptr(states),
                                           dptr(saved), dptr(g_states), dptr(g_mats), dptr(g_root), dptr(gp), dptr(gs), dptr(gd),
                                           stream_handle()), "d3ga_skeleton_bwd")
        if gs is not None and ctx.scale_rows == 1 and B > 1:
            gs = gs.sum(0, keepdim=True)
        return None, None, gp, gs, gd, None, None, None, None


class _MatsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, bind, states):
        require_cuda(bind, states)
        B, J = states.shape[0], states.shape[1]
        mats = torch.empty((B, J, 4, 4), dtype=torch.float32, device=states.device)
        check(_lib.lib().d3ga_skeleton_mats_fwd(B, J, dptr(bind), dptr(states), dptr(mats), stream_handle()),
              "d3ga_skeleton_mats_fwd")
        ctx.save_for_backward(bind, states)
        return mats

    @staticmethod
    def backward(ctx, g):
        bind, states = ctx.saved_tensors
        B, J = states.shape[0], states.shape[1]
        gs = torch.empty_like(states)
        check(_lib.lib().d3ga_skeleton_mats_bwd(B, J, dptr(bind), dptr(states), dptr(g.float().contiguous()), dptr(gs),
                                                stream_handle()), "d3ga_skeleton_mats_bwd")
        return None, gs


def _f32(t):
    return None if t is None else t.float().contiguous()


def _bind_rows(bind_state, J):
    if bind_state.numel() != 8 * J:
        raise ValueError(f"bind_state must be (1,{J},8) or ({J},8), got {tuple(bind_state.shape)}")
    _require_f32("skeleton", bind_state=bind_state)
    return bind_state.detach().reshape(J, 8).contiguous()


def _joint_matrices(bind_state, target_states):
    """(B,J,4,4) through the kernel; target_states (B,J,8)."""
    if target_states.dim() != 3 or target_states.shape[2] != 8:
        raise ValueError(f"target_states must be (B,J,8), got {tuple(target_states.shape)}")
    J = target_states.shape[1]
    return _MatsFn.apply(_bind_rows(bind_state, J), _f32(target_states))


def solve_skeleton_state(param, joint_offset, joint_rotation, joint_parents):
    """(B, 7J) skeleton parameters -> (B,J,8) global joint states, one HIP launch; differentiable in `param`."""
    plan = skeleton_plan(joint_parents, joint_offset, joint_rotation)
    if param.dim() != 2 or param.shape[1] != 7 * plan["J"]:
        raise ValueError(f"param must be (B,{7 * plan['J']}) = 7 values per joint, got {tuple(param.shape)}")
    states, _, _ = _SkeletonFn.apply(plan, None, None, None, _f32(param), 1, False, False, 1.0)
    return states[0]


def states_to_matrix(bind_state, target_states, return_transform=False):
    """(B,J,3,4) joint matrices [R s | t] of target_states against bind_state; differentiable in target_states (the bind state
    is a constant).  return_transform: also (rotation quaternion, translation, scale) of the composed map, in torch."""
    mat = _joint_matrices(bind_state, target_states)[:, :, :3, :]
    if return_transform:
        rel = _relative_states(bind_state, target_states)
        return mat, (rel[..., 3:7], rel[..., 0:3], rel[..., 7:8])
    return mat


# ----------------------------------------------------------------------------------------------------------------------
# modules
# ----------------------------------------------------------------------------------------------------------------------
class ParameterTransform(nn.Module):
    """Pose + scale parameters -> 7 skeleton parameters per joint: transform . p + transform_offsets.  lbs_cfg_dict is what
    `load_momentum_cfg` returns (channel_names, transform (7J,P), transform_offsets (1,7J), limits, nr_scaling_params,
    nr_position_params)."""

    def __init__(self, lbs_cfg_dict):
        super().__init__()
        self.channel_names = list(lbs_cfg_dict["channel_names"])
        self.limits = lbs_cfg_dict["limits"]
        self.nr_scaling_params = lbs_cfg_dict["nr_scaling_params"]
        self.nr_position_params = lbs_cfg_dict["nr_position_params"]
        self.nr_total_params = self.nr_scaling_params + self.nr_position_params
        self.register_buffer("transform_offsets", torch.as_tensor(np.asarray(lbs_cfg_dict["transform_offsets"]), dtype=torch.float32))
        self.register_buffer("transform", torch.as_tensor(np.asarray(lbs_cfg_dict["transform"]), dtype=torch.float32))

    def forward(self, pose):
        """(B, n_params) -> (B, 7J); plain torch (the kernels apply the transform themselves, from its CSR)."""
        return pose @ self.transform.t() + self.transform_offsets


class LinearBlendSkinning(nn.Module):
    """The skeleton and skin of a momentum model file.  model_json: {"Skeleton": {"Bones": [{Name, Parent, PreRotation,
    TranslationOffset}]}, "SkinnedModel": {RestPositions, RestVertexNormals, SkinningWeights [[joint, weight]],
    SkinningOffsets (V+1), Faces {Indices, TextureIndices}, TextureCoordinates}}; a Parent beyond the joint count marks a root."""

    def __init__(self, model_json, lbs_config_dict, num_max_skin_joints=8, scale_path=None):
        super().__init__()
        self.param_transform = ParameterTransform(lbs_config_dict)
        bones = model_json["Skeleton"]["Bones"]
        J = len(bones)
        self.joint_names = [b["Name"] for b in bones]
        parents = np.asarray([-1 if b["Parent"] > J else b["Parent"] for b in bones], dtype=np.int64).reshape(J, 1)
        check_parents(parents)
        rotation = np.asarray([b["PreRotation"] for b in bones], dtype=np.float32).reshape(J, 4)
        offset = np.asarray([b["TranslationOffset"] for b in bones], dtype=np.float32).reshape(J, 3)

        skin = model_json["SkinnedModel"]
        rest = torch.as_tensor(np.asarray(skin["RestPositions"], dtype=np.float32))
        pairs = np.asarray(skin["SkinningWeights"], dtype=np.float64).reshape(-1, 2)
        starts = np.asarray(skin["SkinningOffsets"], dtype=np.int64)
        V, K = len(starts) - 1, num_max_skin_joints
        weights = np.zeros((V, K), dtype=np.float32)
        indices = np.zeros((V, K), dtype=np.int64)
        for k in range(K):                                  # the k-th influence of every vertex that has one
            at = starts[:-1] + k
            has = at < starts[1:]
            weights[has, k] = pairs[at[has], 1]
            indices[has, k] = pairs[at[has], 0].astype(np.int64)

        joint_parents = torch.from_numpy(parents)
        joint_rotation, joint_offset = torch.from_numpy(rotation), torch.from_numpy(offset)
        zero = torch.zeros((1, self.param_transform.nr_total_params), dtype=torch.float32)
        bind_state = solve_skeleton_state_torch(self.param_transform(zero), joint_offset, joint_rotation, joint_parents)

        self.register_buffer("mesh_vertices", rest)
        self.register_buffer("joint_parents", joint_parents)
        self.register_buffer("joint_rotation", joint_rotation)
        self.register_buffer("joint_offset", joint_offset)
        self.register_buffer("mesh_normals", torch.as_tensor(np.asarray(skin["RestVertexNormals"], dtype=np.float32)))
        self.register_buffer("mesh_faces", torch.as_tensor(np.asarray(skin["Faces"]["Indices"], dtype=np.int32)).view(-1, 3))
        self.register_buffer("mesh_texture_faces", torch.as_tensor(np.asarray(skin["Faces"]["TextureIndices"], dtype=np.int32)).view(-1, 3))
        self.register_buffer("mesh_texture_coords", torch.as_tensor(np.asarray(skin["TextureCoordinates"], dtype=np.float32)).view(-1, 2))
        self.register_buffer("skin_weights", torch.from_numpy(weights))
        self.register_buffer("skin_indices", torch.from_numpy(indices))
        self.register_buffer("bind_state", bind_state)
        self.register_buffer("rest_vertices", rest)
        self.register_buffer("joints_weights", self.compute_joints_weights())
        if scale_path is not None:          # a text file of scale parameters, one set per line: the first set, as one row
            self.register_buffer("scale", torch.from_numpy(np.atleast_2d(np.loadtxt(scale_path))[:1].astype(np.float32)))

    @property
    def num_verts(self):
        return self.mesh_vertices.size(0)

    @property
    def num_joints(self):
        return self.joint_offset.size(0)

    @property
    def num_params(self):
        return self.skin_weights.shape[-1]

    # -- HIP path --------------------------------------------------------------------------------------------------------
    def _plan(self):
        pt = self.param_transform
        return skeleton_plan(self.joint_parents, self.joint_offset, self.joint_rotation, pt.transform, pt.transform_offsets)

    def _solve(self, poses, scales=None, n_sets=1, want_mats=True, want_root=False, trans_scale=1.0):
        """-> (states (n_sets,B,J,8), mats (n_sets,B,J,4,4) | None, root (n_sets,B,12) | None).  poses (B, w) are the first w
        parameters, scales (B | 1, n_params - w) the rest (None: zeros)."""
        P = self.param_transform.transform.shape[1]
        if poses.dim() != 2 or poses.shape[1] > P:
            raise ValueError(f"poses must be (B, at most {P} parameters), got {tuple(poses.shape)}")
        ns = P - poses.shape[1]
        if scales is not None:
            if scales.dim() != 2 or scales.shape[1] != ns or scales.shape[0] not in (1, poses.shape[0]):
                raise ValueError(f"poses {tuple(poses.shape)} + scales {tuple(scales.shape)}: the model has {P} parameters, "
                                 f"so scales must be (B | 1, {ns})")
        plan = self._plan()
        bind = _bind_rows(self.bind_state, plan["J"])
        return _SkeletonFn.apply(plan, bind, _f32(poses), _f32(scales), None, n_sets, want_mats, want_root, trans_scale)

    def compute_rigid_transforms(self, global_pose, local_pose, scale):
        """(B,J,8) joint states of the parameters [global_pose | local_pose | scale]."""
        return self._solve(torch.cat([global_pose, local_pose, scale], -1), want_mats=False)[0][0]

    def compute_rigid_transforms_matrix(self, global_pose, local_pose, scale):
        """(B,J,3,4) joint matrices of the parameters [global_pose | local_pose | scale]."""
        return self._solve(torch.cat([global_pose, local_pose, scale], -1))[1][0][:, :, :3, :]

    def compute_root_rigid_transform(self, poses):
        """(t_root (B,3), R_root (B,3,3)): joint 1's matrix with every scale parameter at zero."""
        root = self._solve(poses, None, want_mats=False, want_root=True)[2][0]
        return root[:, 9:12], root[:, :9].reshape(-1, 3, 3)

    def _skin(self, mats, vertices):
        """(B,V,3): lbs_cage per frame over mats (B,J,4,4); vertices (B | 1, V, 3)."""
        B = mats.shape[0]
        if vertices.dim() != 3 or vertices.shape[0] not in (1, B) or vertices.shape[2] != 3:
            raise ValueError(f"vertices must be (B | 1, V, 3), got {tuple(vertices.shape)}")
        _require_f32("skinning", skin_weights=self.skin_weights)
        idx = _i32c(self.skin_indices)
        return torch.stack([lbs_cage(vertices[b if vertices.shape[0] > 1 else 0], None, mats[b], idx, self.skin_weights)
                            for b in range(B)], 0)

    def skinning(self, bind_state, vertices, target_states):
        """Skin `vertices` (B | 1, V, 3) with the joint states target_states (B,J,8) against bind_state (1,J,8)."""
        return self._skin(_joint_matrices(bind_state, target_states), vertices)

    def forward(self, poses, scales, verts_unposed=None):
        """poses (B, n_pose), scales (B | 1, n_scale), verts_unposed (B | 1, V, 3) | None (the rest mesh) -> (B,V,3)."""
        mats = self._solve(poses, scales)[1][0]
        return self._skin(mats, self.mesh_vertices.unsqueeze(0) if verts_unposed is None else verts_unposed)

    # -- set-up paths (plain torch) --------------------------------------------------------------------------------------
    def compute_joints_weights(self, drop_empty=False):
        """Dense (J,V) weights from the K-sparse tables."""
        W = torch.zeros((self.num_joints, self.num_verts), dtype=torch.float32, device=self.skin_weights.device)
        v = torch.arange(self.num_verts, device=self.skin_weights.device)[:, None].expand(-1, self.num_params)
        W[self.skin_indices.long(), v] = self.skin_weights
        return W[W.sum(-1).abs() > 0] if drop_empty else W

    def compute_relative_rigid_transforms(self, global_pose, local_pose, scale):
        """(B,J,7) local translation | rotation of every joint."""
        lt, lq, _ = _local_torch(self.param_transform(torch.cat([global_pose, local_pose, scale], -1)), self.joint_offset,
                                 self.joint_rotation)
        return torch.cat([lt, lq], -1)

    def unpose(self, poses, scales, verts):
        states = solve_skeleton_state_torch(self.param_transform(torch.cat((poses, scales), 1)), self.joint_offset,
                                            self.joint_rotation, self.joint_parents)
        return self.unskinning(self.bind_state, states, verts)

    def unskinning(self, bind_state, target_states, verts):
        """Inverse of `skinning`: every vertex through the inverse of its blended 4x4."""
        mat = states_to_matrix_torch(bind_state, target_states)
        blend = (mat[:, self.skin_indices.long()] * self.skin_weights[None, :, :, None, None]).sum(2)       # (B,V,3,4)
        bottom = blend.new_tensor([0.0, 0.0, 0.0, 1.0]).expand(blend.shape[0], blend.shape[1], 1, 4)
        inv = torch.linalg.inv(torch.cat([blend, bottom], 2))
        hom = torch.cat([verts, torch.ones_like(verts[..., :1])], -1)
        return torch.einsum("bvrc,bvc->bvr", inv, hom)[..., :3].contiguous()


class LBSModule(nn.Module):
    """A subject's body model: the skeleton and skin (`lbs_fn`), the subject's scale parameters, template and global scaling."""

    def __init__(self, lbs_model_json, lbs_config_dict, lbs_template_verts, lbs_scale, global_scaling):
        super().__init__()
        self.lbs_fn = LinearBlendSkinning(lbs_model_json, lbs_config_dict)
        self.register_buffer("lbs_scale", torch.as_tensor(lbs_scale, dtype=torch.float32))
        self.register_buffer("lbs_template_verts", torch.as_tensor(lbs_template_verts, dtype=torch.float32))
        self.register_buffer("global_scaling", torch.as_tensor(global_scaling))

    def _scale(self):
        return self.lbs_scale.reshape(1, -1) if self.lbs_scale.dim() < 2 else self.lbs_scale

    def pose(self, motion, template=None):
        if template is None:
            template = self.lbs_template_verts.reshape(1, -1, 3)
        return self.lbs_fn(motion, self._scale(), template) * self.global_scaling

    def template_pose(self, motion):
        return self.lbs_fn(motion, self._scale(), self.lbs_template_verts.reshape(1, -1, 3)) * self.global_scaling[None]

    def unpose(self, verts, motion):
        scale = self._scale().expand(motion.shape[0], -1)
        return self.lbs_fn.unpose(motion, scale, verts / self.global_scaling) - self.lbs_template_verts


def affine_inverse(M):
    """Inverse of (B,4,4) affine maps [A | t; 0 0 0 1] in closed form (A^-1 from the cross products of A's columns over its
    determinant, then -A^-1 t): a handful of element-wise launches, no solver call, so it neither synchronises nor allocates
    workspace and replays inside a captured graph."""
    c0, c1, c2, t = M[:, :3, 0], M[:, :3, 1], M[:, :3, 2], M[:, :3, 3]
    r0, r1, r2 = torch.cross(c1, c2, dim=-1), torch.cross(c2, c0, dim=-1), torch.cross(c0, c1, dim=-1)
    Ai = torch.stack([r0, r1, r2], 1) / (c0 * r0).sum(-1)[:, None, None]
    ti = -(Ai @ t[..., None])
    bottom = torch.zeros_like(M[:, :1, :])              # filled on the device: no host copy inside a captured graph
    bottom[:, :, 3] = 1.0
    return torch.cat([torch.cat([Ai, ti], 2), bottom], 1)


_template_cache = StorageCache(limit=16)


def _template_dm(t):
    """lbs_template_verts / 100 (the unit of `delta`), cached by the template's storage."""
    return _template_cache.get((t,), None, lambda: (t.detach().float() / 100.0).reshape(-1, 3).contiguous())


_rot180_cache = {}


def default_rot180(device):
    """The half turns about z then y that lib/blueman.py:42-47 applies to the root transform: diag(1, -1, -1, 1), (1,4,4); one
    tensor per device, made on first use (a host copy has no place inside a captured graph)."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    hit = _rot180_cache.get(device)
    if hit is None:
        hit = _rot180_cache[device] = torch.diag(torch.tensor([1.0, -1.0, -1.0, 1.0])).to(device)[None]
    return hit


def goliath_cage(module, motion, delta=None, rot180=None, center_mass=None):
    """What `Blueman.get(motion, return_rt=True, delta=delta)` computes (lib/blueman.py:101-168), on a fixed launch sequence:
    one skeleton launch (the posed solve with the subject's scales and the root solve with zero scales), the (B,4,4) inverse
    in torch (`affine_inverse`; rot180 must be affine), then one skinning launch per frame with global_scaling / 1000, RT and center_mass folded into lbs_cage's Rh / Th.

    module: LBSModule; motion (B, n_pose); delta (V,3) | (1 | B, V, 3) | None, added to lbs_template_verts / 100; rot180
    (1 | B, 4, 4), default `default_rot180`; center_mass broadcastable to (B,1,3), None = no shift.
    -> geom (B,V,3) = RT . (posed / 1000) + center_mass, RT (B,4,4) = inv([R_root | t_root / 1000] . rot180).
    Differentiable in delta and motion."""
    lbs = module.lbs_fn
    B, dev = motion.shape[0], motion.device
    _require_f32("goliath_cage", lbs_template_verts=module.lbs_template_verts, skin_weights=lbs.skin_weights,
                 lbs_scale=module.lbs_scale)
    require_cuda(motion, delta, module.lbs_template_verts, lbs.skin_weights, lbs.skin_indices)
    # translations / 100: the skinning then runs on (template / 100 + delta) and its output is scaled back through Rh
    _, mats, root = lbs._solve(motion, module._scale(), n_sets=2, want_root=True, trans_scale=0.01)
    root = root[1]
    M = torch.zeros((B, 4, 4), dtype=torch.float32, device=dev)
    M[:, :3, :3] = root[:, :9].reshape(B, 3, 3)
    M[:, :3, 3] = root[:, 9:12] / 1000.0
    M[:, 3, 3] = 1.0
    RT = affine_inverse(M @ (default_rot180(dev) if rot180 is None else rot180.to(dev).float()))
    g = module.global_scaling.float().reshape(1, 1, -1) * 0.1          # (global_scaling / 1000) x 100
    Rh = RT[:, :3, :3] * g
    Th = RT[:, :3, 3]
    if center_mass is not None:
        Th = Th + center_mass.to(dev).float().reshape(-1, 3)
    tmpl = _template_dm(module.lbs_template_verts)
    idx = _i32c(lbs.skin_indices)
    if delta is not None:
        delta = delta.reshape(-1, tmpl.shape[0], 3)
        if delta.shape[0] not in (1, B):
            raise ValueError(f"delta must be (V,3) or (1 | B, V, 3) with V = {tmpl.shape[0]}, got {tuple(delta.shape)}")
    geom = torch.stack([lbs_cage(tmpl, None if delta is None else delta[b if delta.shape[0] > 1 else 0], mats[0, b], idx,
                                 lbs.skin_weights, Rh[b], Th[b]) for b in range(B)], 0)
    return geom, RT
