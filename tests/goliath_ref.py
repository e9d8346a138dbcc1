"""Torch restatement of the Goliath skeleton (d3ga_amd/skeleton_model.py docstring) in the dtype of its inputs -- float64 as
the test oracle of the HIP kernels, float32 to measure what that precision alone costs: the parameter transform, the local
transforms, the parent -> child chain as a plain loop over `parents`, the bind-relative joint matrices, 8-sparse skinning, the
root transform and the `Blueman.get` sequence.  Differentiable (autograd).  Quaternions are xyzw and are never normalised."""
import numpy as np
import torch

# Euler angles of the edge set: exact zero, tiny angles, the ordinary range, and up to 6 rad (half angles to 3 rad, past pi/2
# where the cosines change sign)
EDGE_ANGLES = (0.0, 1e-6, -1e-6, 1e-4, 1e-2, 0.35, -1.0, np.pi / 2, 2.0, -np.pi, np.pi + 1e-3, 4.5, -6.0, 6.0)


def qmul(a, b):
    ax, ay, az, aw = a.unbind(-1)
    bx, by, bz, bw = b.unbind(-1)
    return torch.stack([aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx,
                        aw * bz + ax * by - ay * bx + az * bw,
                        aw * bw - ax * bx - ay * by - az * bz], -1)


def qrot(q, v):
    shape = torch.broadcast_shapes(q[..., :3].shape, v.shape)
    a, w, v = q[..., :3].expand(shape), q[..., 3:], v.expand(shape)
    av = torch.cross(a, v, dim=-1)
    return v + 2.0 * (w * av + torch.cross(a, av, dim=-1))


def qinv(q):
    sign = q.new_tensor([-1.0, -1.0, -1.0, 1.0])
    return q * sign / (q * q).sum(-1, keepdim=True)


def euler_quat(r):
    hx, hy, hz = (-0.5 * r[..., 0], 0.5 * r[..., 1], 0.5 * r[..., 2])
    c0, c1, c2, s0, s1, s2 = torch.cos(hx), torch.cos(hy), torch.cos(hz), torch.sin(hx), torch.sin(hy), torch.sin(hz)
    return torch.stack([-s0 * c1 * c2 - c0 * s1 * s2, c0 * s1 * c2 - s0 * c1 * s2, c0 * c1 * s2 + s0 * s1 * c2,
                        c0 * c1 * c2 - s0 * s1 * s2], -1)


def skeleton_params(transform, offsets, poses, scales):
    """(B, 7J) = transform . [poses; scales] + offsets."""
    return torch.cat([poses, scales], 1) @ transform.t() + offsets.reshape(1, -1)


def local_states(param, joint_offset, joint_rotation):
    """(B,J,8) local transforms from (B,7J) skeleton parameters."""
    p = param.reshape(param.shape[0], -1, 7)
    t = p[..., 0:3] + joint_offset
    q = qmul(joint_rotation.expand(p.shape[0], -1, -1), euler_quat(p[..., 3:6]))
    s = torch.exp2(p[..., 6:7])
    return torch.cat([t, q, s], -1)


def chain(P, l):
    """Child state from the parent's state P and the child's local transform l."""
    return torch.cat([qrot(P[..., 3:7], l[..., 0:3] * P[..., 7:8]) + P[..., 0:3], qmul(P[..., 3:7], l[..., 3:7]),
                      P[..., 7:8] * l[..., 7:8]], -1)


def solve(param, joint_offset, joint_rotation, parents):
    """(B,J,8) global states; parents (J,) with -1 at the roots, parents before children."""
    loc = local_states(param, joint_offset, joint_rotation)
    out = []
    for j, p in enumerate(np.asarray(parents).reshape(-1).tolist()):
        out.append(loc[:, j] if p < 0 else chain(out[p], loc[:, j]))
    return torch.stack(out, 1)


def inverse_state(state):
    """The state of the inverse similarity: quaternion inverse through |q|^2, reciprocal scale, translation taken back."""
    qi, si = qinv(state[..., 3:7]), 1.0 / state[..., 7:8]
    return torch.cat([qrot(qi, -state[..., 0:3]) * si, qi, si], -1)


def matrices(bind, states):
    """(B,J,3,4) = [R(q) s | t] of the similarity states . bind^-1, states (B,J,8) against bind (1,J,8) | (J,8)."""
    rel = chain(states, inverse_state(bind.reshape(1, -1, 8)).expand_as(states))
    x, y, z, w = rel[..., 3:7].unbind(-1)
    R = torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     torch.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     torch.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)
    return torch.cat([R * rel[..., 7:8, None], rel[..., 0:3, None]], -1)


def skin(mats, verts, skin_idx, skin_w):
    """(B,V,3) = sum_k w_k M[idx_k] [v;1]; verts (B,V,3) | (1,V,3)."""
    M = mats[:, skin_idx.long()]                                  # (B,V,K,3,4)
    v = verts.expand(mats.shape[0], -1, -1)
    pv = torch.einsum("bvkrc,bvc->bvkr", M[..., :3], v) + M[..., 3]
    return (pv * skin_w[None, :, :, None]).sum(2)


class Rig:
    """A skeleton with its skinning tables, in one dtype.  Arrays: transform (7J,P), offsets (7J,), joint_offset (J,3),
    joint_rotation (J,4), parents (J,), skin_idx (V,K), skin_w (V,K)."""

    def __init__(self, transform, offsets, joint_offset, joint_rotation, parents, skin_idx=None, skin_w=None, dtype=torch.float64):
        t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64)).to(dtype)
        self.dtype = dtype
        self.transform, self.offsets = t(transform), t(offsets).reshape(-1)
        self.joint_offset, self.joint_rotation = t(joint_offset), t(joint_rotation)
        self.parents = np.asarray(parents).reshape(-1).astype(np.int64)
        self.skin_idx = None if skin_idx is None else torch.as_tensor(np.asarray(skin_idx)).long()
        self.skin_w = None if skin_w is None else t(skin_w)
        zero = torch.zeros(1, self.transform.shape[1], dtype=dtype)
        self.bind = solve(zero @ self.transform.t() + self.offsets, self.joint_offset, self.joint_rotation, self.parents)

    def states(self, poses, scales):
        return solve(skeleton_params(self.transform, self.offsets, poses, scales), self.joint_offset, self.joint_rotation,
                     self.parents)

    def mats(self, poses, scales):
        return matrices(self.bind, self.states(poses, scales))

    def forward(self, poses, scales, verts):
        return skin(self.mats(poses, scales), verts, self.skin_idx, self.skin_w)

    def root(self, poses, root_joint=1):
        """(t_root (B,3), R_root (B,3,3)): the root joint's matrix of the solve with zero scales."""
        z = poses.new_zeros(poses.shape[0], self.transform.shape[1] - poses.shape[1])
        m = self.mats(poses, z)
        return m[:, root_joint, :, 3], m[:, root_joint, :, :3]

    def cage(self, motion, scale, template, global_scaling, rot180, center_mass, delta=None):
        """The `Blueman.get` sequence: pose (template in the rig's units, delta in units 100 times larger), root solve, RT =
        inv([R | t / 1000] rot180), geom = RT . (posed / 1000) + center_mass.  -> (geom (B,V,3), RT (B,4,4))."""
        B = motion.shape[0]
        tmpl = template.reshape(1, -1, 3).expand(B, -1, -1)
        if delta is not None:
            tmpl = (tmpl / 100.0 + delta.reshape(-1, tmpl.shape[1], 3).expand(B, -1, -1)) * 100.0
        geom = self.forward(motion, scale.reshape(1, -1).expand(B, -1), tmpl) * global_scaling
        t_root, R_root = self.root(motion)
        RT = torch.eye(4, dtype=self.dtype).repeat(B, 1, 1)
        RT[:, :3, :3] = R_root
        RT[:, :3, 3] = t_root / 1000.0
        RT = torch.linalg.inv(RT @ rot180)
        geom = geom / 1000.0
        geom = geom @ RT[:, :3, :3].transpose(1, 2) + RT[:, None, :3, 3]
        return geom + center_mass, RT


def random_tree(rng, J, kind):
    """parents (J,) with the parent-first property and parents[0] = -1: "chain", "star" (every joint on joint 0), "bushy", or
    "forest" (bushy, with about every eighth joint a further root)."""
    par = np.full(J, -1, dtype=np.int64)
    for j in range(1, J):
        if kind == "forest" and rng.random() < 0.125:
            continue
        par[j] = j - 1 if kind == "chain" else 0 if kind == "star" else int(rng.integers(max(0, j - 6), j))
    return par


def random_rig(rng, J, n_pose, n_scale, kind="bushy", V=0, K=8, max_depth=None, t_mag=1.0, unused=0, dtype=torch.float64):
    """A seeded rig.  Rotation and translation rows of the transform draw on pose parameters, scale rows on scale parameters
    (2 nonzeros per row at most, some rows empty); `unused` trailing pose parameters are read by no joint."""
    par = random_tree(rng, J, kind)
    if max_depth is not None:                      # cap the chain depth: re-hang joints that sit too deep
        depth = np.zeros(J, dtype=np.int64)
        for j in range(1, J):
            if par[j] < 0:
                continue                           # a further root
            if depth[par[j]] + 1 > max_depth:
                shallow = np.flatnonzero(depth[:j] < max_depth)
                par[j] = int(shallow[rng.integers(0, len(shallow))])
            depth[j] = depth[par[j]] + 1
    P = n_pose + n_scale
    T = np.zeros((7 * J, P))
    used = max(1, n_pose - unused)
    for r in range(7 * J):
        if rng.random() < 0.25:
            continue                               # an empty row: the parameter is its offset alone
        cols = rng.integers(0, n_scale, size=rng.integers(1, 3)) + n_pose if (r % 7 == 6 and n_scale > 0) else \
            rng.integers(0, used, size=rng.integers(1, 3))
        for c in cols:
            T[r, c] = (1.0, -1.0, 0.5, rng.uniform(-1.0, 1.0))[rng.integers(0, 4)]      # unit coefficients keep edge angles exact
    off = rng.normal(size=7 * J) * 0.05
    joff = rng.normal(size=(J, 3)) * t_mag
    jrot = rng.normal(size=(J, 4))
    jrot /= np.linalg.norm(jrot, axis=1, keepdims=True)
    idx = w = None
    if V:
        idx = rng.integers(0, J, size=(V, K))
        w = rng.random((V, K))
        w[:, 5:] = 0.0
        w /= w.sum(1, keepdims=True)
    return Rig(T.astype(np.float32), off.astype(np.float32), joff.astype(np.float32), jrot.astype(np.float32), par, idx,
               None if w is None else w.astype(np.float32), dtype=dtype)


def rig_json(joint_offset, joint_rotation, parents, skin_idx, skin_w, rest):
    """A momentum-style model dict (the constructor input of LinearBlendSkinning) from plain arrays; influences with weight 0
    are left out of the per-vertex lists, a root's Parent is a number beyond the joint count."""
    J = len(parents)
    bones = [dict(Name=f"joint{j}", Parent=int(parents[j]) if parents[j] >= 0 else 2 ** 31 - 1,
                  PreRotation=[float(x) for x in joint_rotation[j]], TranslationOffset=[float(x) for x in joint_offset[j]])
             for j in range(J)]
    pairs, starts = [], [0]
    for v in range(len(skin_idx)):
        for k in range(skin_idx.shape[1]):
            if skin_w[v, k] != 0:
                pairs.append([int(skin_idx[v, k]), float(skin_w[v, k])])
        starts.append(len(pairs))
    V = len(rest)
    return dict(Skeleton=dict(Bones=bones),
                SkinnedModel=dict(RestPositions=[[float(x) for x in r] for r in rest], RestVertexNormals=[[0.0, 0.0, 1.0]] * V,
                                  SkinningWeights=pairs, SkinningOffsets=starts,
                                  Faces=dict(Indices=[0, 1, 2], TextureIndices=[0, 1, 2]),
                                  TextureCoordinates=[0.0, 0.0, 1.0, 0.0, 0.0, 1.0]))


def rig_config(transform, offsets, n_pose, n_scale):
    """The lbs_config_dict of ParameterTransform for a dense transform."""
    return dict(channel_names=["tx", "ty", "tz", "rx", "ry", "rz", "sc"], transform=np.asarray(transform, dtype=np.float32),
                transform_offsets=np.asarray(offsets, dtype=np.float32).reshape(1, -1), limits=[], nr_scaling_params=n_scale,
                nr_position_params=n_pose)


# ----------------------------------------------------------------------------------------------------------------------
# fuzz cases (tests/test_gpu_skeleton.py; their float32 margin is checked on the CPU in tests/test_skeleton_host.py)
# ----------------------------------------------------------------------------------------------------------------------
FUZZ_MAX_DEPTH = 24          # deepest parent chain (the Goliath rig: below 20); deeper random chains are re-hung
FUZZ_SCALE_MAG = 0.15        # scale parameters in [-0.15, 0.15]: a joint's log2 scale stays within about +-0.4
FUZZ_T_MAG = 1.0             # joint offsets ~ N(0, 1)


def fuzz_case(seed):
    """One seeded case: a rig of 2..256 joints (chain / star / bushy / forest of several roots), a sparse transform with parameters no joint uses, pose
    values from EDGE_ANGLES, a subset of the upstream gradients (states, matrices, root; never none), scales of one row or B."""
    rng = np.random.default_rng(seed)
    J = int((2, 3, 7, 64, 65, 160, 255, 256)[rng.integers(0, 8)]) if rng.random() < 0.5 else int(rng.integers(2, 257))
    kind = ("chain", "star", "bushy", "forest")[rng.integers(0, 4)]
    n_pose, n_scale = int(rng.integers(1, 40)), int(rng.integers(0, 6))
    B = int((1, 1, 2, 3, 5)[rng.integers(0, 5)])
    rig = random_rig(rng, J, n_pose, n_scale, kind=kind, V=int(rng.integers(1, 40)), max_depth=FUZZ_MAX_DEPTH, t_mag=FUZZ_T_MAG,
                     unused=int(rng.integers(0, 3)))
    poses = np.asarray(EDGE_ANGLES)[rng.integers(0, len(EDGE_ANGLES), size=(B, n_pose))] * rng.choice([-1.0, 1.0], size=(B, n_pose))
    scales = rng.uniform(-FUZZ_SCALE_MAG, FUZZ_SCALE_MAG, size=(1 if rng.random() < 0.5 else B, n_scale))
    use = rng.random(3) < 0.5
    if not use.any():
        use[rng.integers(0, 3)] = True
    return dict(seed=seed, rig=rig, J=J, kind=kind, B=B, poses=poses.astype(np.float32), scales=scales.astype(np.float32),
                use_states=bool(use[0]), use_mats=bool(use[1]), use_root=bool(use[2]),
                g_states=rng.normal(size=(B, J, 8)).astype(np.float32), g_mats=rng.normal(size=(B, J, 3, 4)).astype(np.float32),
                g_root=rng.normal(size=(B, 12)).astype(np.float32))


def fuzz_eval(case, dtype):
    """The case through the formulae above in `dtype` -> dict of numpy float64 arrays: states, mats, root (B,12) = [R | t] of the
    zero-scale solve, and the gradients of the case's upstream subset w.r.t. poses and scales."""
    r = case["rig"]
    rig = Rig(r.transform, r.offsets, r.joint_offset, r.joint_rotation, r.parents, dtype=dtype)
    poses = torch.tensor(case["poses"], dtype=dtype, requires_grad=True)
    scales = torch.tensor(case["scales"], dtype=dtype, requires_grad=True)
    B = poses.shape[0]
    states = rig.states(poses, scales.expand(B, -1))
    mats = matrices(rig.bind, states)
    t_root, R_root = rig.root(poses, root_joint=min(1, rig.parents.size - 1))
    root = torch.cat([R_root.reshape(B, 9), t_root], 1)
    loss = poses.sum() * 0
    if case["use_states"]:
        loss = loss + (states * torch.tensor(case["g_states"], dtype=dtype)).sum()
    if case["use_mats"]:
        loss = loss + (mats * torch.tensor(case["g_mats"], dtype=dtype)).sum()
    if case["use_root"]:
        loss = loss + (root * torch.tensor(case["g_root"], dtype=dtype)).sum()
    gp, gs = torch.autograd.grad(loss, [poses, scales], allow_unused=True)
    f = lambda t: None if t is None else t.detach().double().numpy()
    return dict(states=f(states), mats=f(mats), root=f(root), g_poses=f(gp), g_scales=f(torch.zeros_like(scales) if gs is None else gs))


def free_case(seed):
    """A case for the free functions (skeleton parameters handed over as they are): the rig of fuzz_case(seed), B frames with
    B x J on either side of a multiple of 256, translations and log2 scales within FUZZ_SCALE_MAG, angles from EDGE_ANGLES."""
    case = fuzz_case(seed)
    J = case["J"]
    rng = np.random.default_rng(seed)
    B = int((1, 2, 3, 7, 16)[rng.integers(0, 5)])
    param = rng.uniform(-FUZZ_SCALE_MAG, FUZZ_SCALE_MAG, size=(B, J, 7))
    param[:, :, 3:6] = np.asarray(EDGE_ANGLES)[rng.integers(0, len(EDGE_ANGLES), size=(B, J, 3))] * rng.choice([-1.0, 1.0], size=(B, J, 3))
    return dict(seed=seed, rig=case["rig"], J=J, kind=case["kind"], B=B, param=param.reshape(B, 7 * J).astype(np.float32),
                use_states=bool(rng.random() < 0.5), g_states=rng.normal(size=(B, J, 8)).astype(np.float32),
                g_mats=rng.normal(size=(B, J, 3, 4)).astype(np.float32))


def free_eval(case, dtype):
    """solve + matrices on the case in `dtype` (the bind state rounded to float32 first, as the kernels are handed it) ->
    dict of numpy float64 arrays: states, mats, g_param."""
    r = case["rig"]
    t = lambda x: torch.as_tensor(x).to(dtype)
    param = torch.tensor(case["param"], dtype=dtype, requires_grad=True)
    states = solve(param, t(r.joint_offset), t(r.joint_rotation), r.parents)
    mats = matrices(r.bind.float().to(dtype), states)
    loss = (mats * t(case["g_mats"])).sum() + ((states * t(case["g_states"])).sum() if case["use_states"] else 0)
    (g,) = torch.autograd.grad(loss, [param])
    f = lambda x: x.detach().double().numpy()
    return dict(states=f(states), mats=f(mats), g_param=f(g))
