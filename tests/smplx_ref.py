"""Float64 torch restatement of the SMPL / SMPL-X layer (d3ga_amd/body_model.py docstring), straight from the raw model
arrays: the pose layouts and hand PCA, shape / expression / pose blend shapes, joint regression, forward kinematics as a
plain loop over `parents`, and linear blend skinning.  The test oracle of the HIP kernels; differentiable (autograd)."""
import numpy as np
import torch


def _t(x, dtype):
    if hasattr(x, "toarray"):
        x = x.toarray()
    return torch.as_tensor(np.asarray(x, dtype=np.float64)).to(dtype)


def rodrigues(r, eps=1e-8):
    t = torch.linalg.norm(r + eps, dim=1, keepdim=True)
    k = r / t
    s, c = torch.sin(t)[:, :, None], torch.cos(t)[:, :, None]
    z = torch.zeros_like(k[:, 0])
    K = torch.stack([z, -k[:, 2], k[:, 1], k[:, 2], z, -k[:, 0], -k[:, 1], k[:, 0], z], dim=1).view(-1, 3, 3)
    eye = torch.eye(3, dtype=r.dtype, device=r.device)[None]
    return eye + s * K + (1.0 - c) * torch.bmm(K, K)


# |theta| of the rotation edge set: exact zero, tiny angles where t = |theta + 1e-8| is dominated by the offset, the
# ordinary range, and the points where sin / cos change sign or the axis-angle wraps (pi, 2 pi and beyond).
EDGE_ANGLES = (0.0, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 0.35, 1.0, np.pi / 2, np.pi - 1e-3, np.pi, np.pi + 1e-3, 4.0,
               2 * np.pi - 1e-3, 2 * np.pi, 2 * np.pi + 1e-3)


def edge_rotations(rng, n):
    """(n, 3) float32 axis-angle vectors over EDGE_ANGLES (cycled), each on a random axis, a coordinate axis (zero
    components) or a negative coordinate axis."""
    out = np.zeros((n, 3))
    for i in range(n):
        a = EDGE_ANGLES[i % len(EDGE_ANGLES)]
        kind = (i // len(EDGE_ANGLES)) % 3
        if kind == 0:
            d = rng.normal(size=3)
            d /= np.linalg.norm(d)
        else:
            d = np.zeros(3)
            d[int(rng.integers(0, 3))] = 1.0 if kind == 1 else -1.0
        out[i] = a * d
    return out.astype(np.float32)


class RefSMPL:
    def __init__(self, data, model_type="smplx", num_pca_comps=6, use_flat_mean=True, dtype=torch.float64, device="cpu"):
        kw = dict(dtype=dtype)
        self.vt = _t(data["v_template"], dtype).to(device)
        V = self.vt.shape[0]
        sd = _t(data["shapedirs"], dtype).reshape(V, 3, -1)
        if model_type == "smplx":
            e0 = 300 if sd.shape[2] == 400 else 10
            self.sdirs = torch.cat([sd[:, :, :10], sd[:, :, e0:e0 + 10]], dim=2).to(device)
            self.n_expr = 10
        else:
            self.sdirs = sd[:, :, :10].to(device)
            self.n_expr = 0
        self.pdirs = _t(data["posedirs"], dtype).reshape(V, 3, -1).to(device)
        self.Jreg = _t(data["J_regressor"], dtype).to(device)
        self.W = _t(data["weights"], dtype).to(device)
        p = np.asarray(data["kintree_table"]).astype(np.int64)[0].copy()
        p[0] = -1
        self.parents = [int(x) for x in p]
        self.J = len(self.parents)
        self.model_type, self.npca = model_type, num_pca_comps
        if model_type == "smplx":
            self.hc = [_t(data["hands_components" + s], dtype)[:num_pca_comps].to(device) for s in ("l", "r")]
            self.hm = [torch.zeros(45, **kw).to(device) if use_flat_mean else _t(data["hands_mean" + s], dtype).to(device)
                       for s in ("l", "r")]
        self.NUM_POSES = 75 + 2 * num_pca_comps if model_type == "smplx" and num_pca_comps > 0 else 3 * self.J

    def full_pose(self, poses):
        if poses.shape[1] == 3 * self.J:
            return poses
        n = self.npca
        body, lh, rh, face = poses[:, :66], poses[:, 66:66 + n], poses[:, 66 + n:66 + 2 * n], poses[:, 66 + 2 * n:]
        return torch.cat([body, face, lh @ self.hc[0] + self.hm[0], rh @ self.hc[1] + self.hm[1]], dim=1)

    def __call__(self, poses, shapes, Rh=None, Th=None, expression=None):
        B = poses.shape[0]
        dt = self.vt.dtype
        if shapes.shape[0] != B:
            shapes = shapes.expand(B, -1)
        shapes = torch.nn.functional.pad(shapes, (0, 10 - shapes.shape[1]))      # fewer coefficients: the rest are zero
        coef = shapes
        if self.n_expr:
            e = expression if expression is not None else torch.zeros(B, 10, dtype=dt, device=poses.device)
            if e.shape[0] != B:
                e = e.expand(B, -1)
            e = torch.nn.functional.pad(e, (0, 10 - e.shape[1]))
            coef = torch.cat([shapes, e], dim=1)
        th = self.full_pose(poses).reshape(B * self.J, 3)
        R = rodrigues(th).view(B, self.J, 3, 3)
        eye = torch.eye(3, dtype=dt, device=poses.device)
        pf = (R[:, 1:] - eye).reshape(B, -1)
        bs = torch.einsum("vcs,bs->bvc", self.sdirs, coef) + torch.einsum("vcp,bp->bvc", self.pdirs, pf)
        v_shaped = self.vt[None] + torch.einsum("vcs,bs->bvc", self.sdirs, coef)
        Jr = torch.einsum("jv,bvc->bjc", self.Jreg, v_shaped)
        G = [None] * self.J
        bottom = torch.tensor([0, 0, 0, 1], dtype=dt, device=poses.device).expand(B, 1, 4)
        for j in range(self.J):
            p = self.parents[j]
            t = Jr[:, j] if p < 0 else Jr[:, j] - Jr[:, p]
            L = torch.cat([torch.cat([R[:, j], t[:, :, None]], dim=2), bottom], dim=1)
            G[j] = L if p < 0 else G[p] @ L
        G = torch.stack(G, dim=1)                                            # (B,J,4,4)
        tj = torch.einsum("bjrc,bjc->bjr", G[:, :, :3, :3], Jr)
        A = torch.cat([torch.cat([G[:, :, :3, :3], (G[:, :, :3, 3] - tj)[..., None]], dim=3),
                       bottom[:, None].expand(B, self.J, 1, 4)], dim=2)
        T = torch.einsum("vj,bjk->bvk", self.W, A.reshape(B, self.J, 16)).reshape(B, -1, 4, 4)
        vp = self.vt[None] + bs
        u = torch.einsum("bvrc,bvc->bvr", T[:, :, :3, :3], vp) + T[:, :, :3, 3]
        if Rh is not None:
            u = u @ rodrigues(Rh).transpose(1, 2)
        if Th is not None:
            u = u + Th[:, None]
        return u, T, A, bs
