"""The SMPL / SMPL-X body model: `tetra_sampler.body_model.SMPLlayer` as the reference builds and calls it
(lib/smplman.py:68-74, 175), evaluated by the HIP kernels of csrc/body_model.hip (include/d3ga.h, B1).

The layer follows EasyMocap's `SMPLlayer`, from which tetra-sampler's descends.  tetra-sampler is un-vendored, so nothing
reference-held pins the conventions below: they are RESTATED, UNPINNED (as `cage_deform.batch_rodrigues` is), from the
published SMPL / SMPL-X model definition.

Model files (licensed; the user downloads them, `config.data.smplx_model`): `model_path` is a `.pkl` (latin-1 pickle) or
`.npz` file, or a directory holding `SMPLX_{GENDER}.{pkl,npz}` (`SMPL_{GENDER}` for model_type="smpl").  Keys read:
v_template (V,3), shapedirs (V,3,S), posedirs (V,3,9(J-1)), J_regressor (J,V), weights (V,J), kintree_table (2,J), f, and for
SMPL-X hands_components{l,r} (45,45), hands_mean{l,r} (45).  Arrays may be numpy or scipy.sparse; chumpy objects are refused.

Coefficients: 10 shape components (shapedirs[..., :10]); SMPL-X adds 10 expression components, shapedirs[..., 300:310] when
S = 400 or [..., 10:20] when S = 20.

Pose vectors, (B, NUM_POSES) or the full (B, 3J):
  SMPL:    72 = 24 joints x axis-angle.
  SMPL-X:  NUM_POSES = 87 with the defaults num_pca_comps=6, use_pca=True, use_flat_mean=True:
             [body 0:66 | left-hand PCA 66:72 | right-hand PCA 72:78 | jaw, left eye, right eye 78:87]
           hand = PCA coefficients . hands_components[:6] (+ hands_mean unless use_flat_mean);
           the full 165 is the joint order [body 66 | jaw, leye, reye 9 | left hand 45 | right hand 45]
           (datasets/actorshq_dataset.py:59).  num_pca_comps is 0..45; with 45 the compact width is 165 as well, and a
           165-wide pose is then read as the full layout (a 3J-wide pose always is).

Per frame: R_j = Rodrigues(theta_j) (t = |theta_j + 1e-8|), pose feature pf = (R_j - I), j >= 1, row-major;
bs = shapedirs [beta; psi] + posedirs pf (= v_posed - v_template); rest joints J = J_regressor (v_template + shapedirs
[beta; psi]); forward kinematics over `parents`; A_j = [RG_j | tG_j - RG_j J_j]; T_v = sum_j w_vj A_j;
verts = (T_v [v_template + bs; 1]) R(Rh)^T + Th.  `forward` returns (verts, T, A, bs) -- A and T without Rh / Th, which
Smplman.deform applies itself (lib/smplman.py:166-169)."""
import ctypes
import os
import pickle

import numpy as np
import torch

from . import _lib
from ._lib import check, dptr, f32c16, require_cuda, stream_handle


class ModelFileNotFoundError(FileNotFoundError, NotImplementedError):
    """The SMPL-X / SMPL model file is missing.  A NotImplementedError as well, for callers that treat the body model as
    an optional piece (the licensed assets are not part of this project)."""


def _gender_name(gender):
    return str(gender).upper()


def find_model_file(model_path, model_type="smplx", gender="neutral"):
    """The model file `model_path` names: itself when it is a file, else SMPLX_{GENDER}.pkl / .npz (SMPL_ for "smpl") in it."""
    if model_type not in ("smplx", "smpl"):
        raise ValueError(f"SMPLlayer: model_type {model_type!r} is not supported (smplx | smpl; SMPL-H is not)")
    path = os.fspath(model_path) if model_path is not None else ""
    if os.path.isfile(path):
        return path
    stem = ("SMPLX_" if model_type == "smplx" else "SMPL_") + _gender_name(gender)
    tried = [os.path.join(path, stem + ext) for ext in (".pkl", ".npz")] if path else []
    for p in tried:
        if os.path.isfile(p):
            return p
    raise ModelFileNotFoundError(
        f"SMPL-X body model file not found (model_type={model_type!r}, gender={gender!r}): tried {path!r}"
        + (" and " + ", ".join(repr(p) for p in tried) if tried else "")
        + ".  The SMPL-X / SMPL model files are licensed and not part of d3ga_amd: download them and point "
          "config.data.smplx_model at the file or its directory.")


class _NoChumpy(pickle.Unpickler):
    def find_class(self, module, name):
        if module.split(".")[0] == "chumpy":
            raise ValueError(
                f"this SMPL model pickle holds chumpy objects ({module}.{name}); chumpy pickles are not supported. Convert "
                "the model to plain numpy arrays first (load it once where chumpy is installed and save every array with "
                "np.asarray, e.g. to .npz).")
        return super().find_class(module, name)


def load_model_data(path):
    """Raw arrays of a model file as a dict (numpy or scipy.sparse values)."""
    if path.endswith(".npz"):
        with np.load(path, allow_pickle=True) as z:
            return {k: z[k] for k in z.files}
    with open(path, "rb") as f:
        data = _NoChumpy(f, encoding="latin1").load()
    if not isinstance(data, dict):
        raise ValueError(f"{path}: expected a dict of arrays, got {type(data).__name__}")
    return dict(data)


def _dense(x):
    if hasattr(x, "toarray"):          # scipy.sparse
        x = x.toarray()
    return np.asarray(x, dtype=np.float64)


def tree_tables(parents):
    """Level table (level_ptr, level_joint) and children CSR (child_ptr, child_joint) of a kinematic tree; parents[0] = -1."""
    J = len(parents)
    depth = np.full(J, -1, dtype=np.int64)
    for j in range(J):
        chain, k = [], j
        while k >= 0 and depth[k] < 0:
            chain.append(k)
            k = int(parents[k])
            if len(chain) > J:
                raise ValueError("kintree_table is not a tree (cycle)")
        d = -1 if k < 0 else depth[k]
        for q in reversed(chain):
            d += 1
            depth[q] = d
    order = np.lexsort((np.arange(J), depth))
    n_levels = int(depth.max()) + 1
    level_ptr = np.searchsorted(depth[order], np.arange(n_levels + 1)).astype(np.int32)
    kids = [j for j in range(J) if parents[j] >= 0]
    kids.sort(key=lambda j: (parents[j], j))
    child_ptr = np.zeros(J + 1, dtype=np.int32)
    for j in kids:
        child_ptr[parents[j] + 1] += 1
    child_ptr = np.cumsum(child_ptr).astype(np.int32)
    return level_ptr, order.astype(np.int32), child_ptr, np.asarray(kids, dtype=np.int32), depth


def prepare(data, model_type="smplx", num_pca_comps=6, use_pca=True, use_flat_mean=True, n_shape=10, n_expr=10):
    """Kernel layouts of a model (numpy; products in float64, stored as float32 / int32).  Returns a dict."""
    need = ["v_template", "shapedirs", "posedirs", "J_regressor", "weights", "kintree_table", "f"]
    miss = [k for k in need if k not in data]
    if miss:
        raise ValueError(f"SMPL model data lacks {miss}")
    if not 0 <= num_pca_comps <= 45:
        raise ValueError(f"num_pca_comps={num_pca_comps}: the hand PCA has 45 components per hand (0..45)")
    parents = np.asarray(data["kintree_table"]).astype(np.int64)[0].copy()
    parents[0] = -1
    J = len(parents)
    if J > _lib.BODY_MAX_JOINTS:
        raise ValueError(f"{J} joints: the kernels take at most {_lib.BODY_MAX_JOINTS}")
    if J < 2:
        raise ValueError(f"{J} joint: the kernels take at least 2 (a rigid body is the global Rh / Th of any model)")
    vt = _dense(data["v_template"])
    V = vt.shape[0]
    sd = _dense(data["shapedirs"]).reshape(V, 3, -1)
    pd = _dense(data["posedirs"]).reshape(V, 3, -1)
    Jreg = _dense(data["J_regressor"])
    W = _dense(data["weights"])
    if Jreg.shape != (J, V) or W.shape != (V, J) or pd.shape[2] != 9 * (J - 1):
        raise ValueError(f"inconsistent SMPL model: V={V}, J={J}, J_regressor {Jreg.shape}, weights {W.shape}, posedirs {pd.shape}")
    S = sd.shape[2]
    if model_type == "smplx":
        if S == 400:
            e0 = 300
        elif S == 20:
            e0 = 10
        else:
            raise ValueError(f"SMPL-X shapedirs with {S} components: expected 400 (300 shape + 100 expression) or 20")
        dirs_se = np.concatenate([sd[:, :, :n_shape], sd[:, :, e0:e0 + n_expr]], axis=2)
    else:
        n_expr = 0
        dirs_se = sd[:, :, :n_shape]
    NS = n_shape + n_expr
    if dirs_se.shape[2] != NS:
        raise ValueError(f"shapedirs has {S} components, {NS} needed")
    NP = 9 * (J - 1)
    ld = -(-3 * V // _lib.BODY_LD_ALIGN) * _lib.BODY_LD_ALIGN
    dirs = np.zeros((NS + NP, ld), dtype=np.float32)
    dirs[:NS, :3 * V] = dirs_se.reshape(3 * V, NS).T
    dirs[NS:, :3 * V] = pd.reshape(3 * V, NP).T
    J0 = Jreg @ vt
    Jdirs = np.einsum("jv,vcs->sjc", Jreg, dirs_se)
    rows, cols = np.nonzero(W)                       # every nonzero, row-major: CSR by vertex
    w_ptr = np.searchsorted(rows, np.arange(V + 1)).astype(np.int32)
    ordj = np.lexsort((rows, cols))                  # by joint, vertices ascending
    wt_ptr = np.searchsorted(cols[ordj], np.arange(J + 1)).astype(np.int32)
    level_ptr, level_joint, child_ptr, child_joint, depth = tree_tables(parents)
    out = dict(V=V, J=J, n_shape=n_shape, n_expr=n_expr, ld=ld, parents=parents.astype(np.int32), depth=depth,
               v_template=vt.astype(np.float32), dirs=dirs, J0=J0.astype(np.float32), Jdirs=Jdirs.astype(np.float32),
               w_ptr=w_ptr, w_joint=cols.astype(np.int32), w_val=W[rows, cols].astype(np.float32),
               wt_ptr=wt_ptr, wt_vert=rows[ordj].astype(np.int32), wt_val=W[rows[ordj], cols[ordj]].astype(np.float32),
               level_ptr=level_ptr, level_joint=level_joint, child_ptr=child_ptr, child_joint=child_joint,
               weights=W.astype(np.float32), J_regressor=Jreg.astype(np.float32),
               faces=np.asarray(data["f"]).astype(np.int64), n_hand_pca=0)
    if model_type == "smplx":
        if J != 55:
            raise ValueError(f"SMPL-X has 55 joints, the model file {J}")
        if not use_pca:
            num_pca_comps = 0
        if num_pca_comps > 0:
            comps, means = [], []
            for side in ("l", "r"):
                c = _dense(data["hands_components" + side])[:num_pca_comps]
                m = _dense(data["hands_mean" + side]).reshape(45)
                comps.append(c)
                means.append(np.zeros_like(m) if use_flat_mean else m)
            out["hand_comps"] = np.stack(comps).astype(np.float32)
            out["hand_mean"] = np.stack(means).astype(np.float32)
            out["n_hand_pca"] = num_pca_comps
    return out


_KERNEL_BUFFERS = ("dirs", "w_ptr", "w_joint", "w_val", "wt_ptr", "wt_vert", "wt_val", "J0", "Jdirs", "parents", "level_ptr",
                   "level_joint", "child_ptr", "child_joint", "hand_comps", "hand_mean")


class SMPLlayer(torch.nn.Module):
    """`tetra_sampler.body_model.SMPLlayer(model_path, model_type, gender, use_joints, regressor_path)`: the SMPL-X (or
    SMPL) body model on the HIP kernels.  See the module docstring for the files, the pose layouts and the math.

    forward(poses, shapes, Rh=None, Th=None, expression=None, return_verts=True) -> (verts, T, A, bs):
    verts (B,V,3), T (B,V,4,4), A (B,J,4,4), bs (B,V,3); differentiable in poses, shapes, expression, Rh and Th.  `shapes`
    and `expression` of one row are broadcast over the batch (their gradient is then summed over it).  With
    return_verts=False the first output is keypoints (B,K,3) = regressor . verts, the regressor from `regressor_path`
    (.npy dense (K,V), or .txt `row col value` triplets with an optional `# K V` header) or J_regressor without one."""

    def __init__(self, model_path=None, model_type="smplx", gender="neutral", use_joints=True, regressor_path=None,
                 num_pca_comps=6, use_pca=True, use_flat_mean=True, **kw):
        super().__init__()
        path = find_model_file(model_path, model_type, gender)
        m = prepare(load_model_data(path), model_type, num_pca_comps, use_pca, use_flat_mean)
        self.model_type, self.gender, self.use_joints, self.regressor_path = model_type, gender, use_joints, regressor_path
        self.V, self.J, self.n_shape, self.n_expr, self.ld = m["V"], m["J"], m["n_shape"], m["n_expr"], m["ld"]
        self.n_hand_pca, self.n_levels = m["n_hand_pca"], len(m["level_ptr"]) - 1
        self.NUM_POSES = 3 * self.J if self.n_hand_pca == 0 else 75 + 2 * self.n_hand_pca
        self.register_buffer("faces_tensor", torch.from_numpy(m["faces"]))
        self.register_buffer("v_template", torch.from_numpy(m["v_template"]))
        self.register_buffer("weights", torch.from_numpy(m["weights"]))
        self.register_buffer("J_regressor", torch.from_numpy(m["J_regressor"]))
        for k in _KERNEL_BUFFERS:
            a = m.get(k)
            if a is not None and a.size == 0:       # no skin weight at all: an empty tensor's device pointer is NULL, which
                a = np.zeros(1, a.dtype)            # the C ABI refuses; the empty CSR ranges never read this element
            self.register_buffer("bm_" + k, None if a is None else torch.from_numpy(np.ascontiguousarray(a)), persistent=False)
        self._struct = None
        self._struct_key = None
        self._kp_regressor = None

    # ------------------------------------------------------------------------------------------------------------------
    def model_struct(self):
        """struct d3ga_body_model over the current device buffers (rebuilt when the module moves)."""
        key = tuple(t.data_ptr() if t is not None else 0 for t in [self.v_template] + [getattr(self, "bm_" + k) for k in _KERNEL_BUFFERS])
        if key != self._struct_key:
            bufs = [("v_template", self.v_template)] + [("bm_" + k, getattr(self, "bm_" + k)) for k in _KERNEL_BUFFERS]
            bad = [f"{k} {t.dtype}" for k, t in bufs if t is not None and t.dtype not in (torch.float32, torch.int32)]
            if bad:
                raise TypeError(f"SMPLlayer: the kernels read float32 model buffers, these are not: {', '.join(bad)}.  "
                                "Keep the layer in float32 (no .double() / .half()); the inputs may be of any float dtype.")
            s = _lib.BodyModel(V=self.V, J=self.J, n_shape=self.n_shape, n_expr=self.n_expr, n_hand_pca=self.n_hand_pca,
                               ld=self.ld, n_levels=self.n_levels, reserved=0)
            s.v_template = self.v_template.data_ptr()
            for k in _KERNEL_BUFFERS:
                t = getattr(self, "bm_" + k)
                setattr(s, k, t.data_ptr() if t is not None else None)
            self._struct, self._struct_key = s, key
        return self._struct

    def scratch_bytes(self, B):
        f, b = ctypes.c_int64(), ctypes.c_int64()
        check(_lib.lib().d3ga_body_model_scratch_bytes(ctypes.byref(self.model_struct()), B, ctypes.byref(f), ctypes.byref(b)),
              "d3ga_body_model_scratch_bytes")
        return f.value, b.value

    def _coef(self, x, n, B, what):
        if x is None:
            return None
        if x.dim() != 2 or x.shape[1] > n or x.shape[0] not in (1, B):
            raise ValueError(f"SMPLlayer: {what} must be (B,{n}) or (1,{n}), got {tuple(x.shape)}")
        x = x.float()
        if x.shape[1] < n:
            x = torch.nn.functional.pad(x, (0, n - x.shape[1]))
        if x.shape[0] != B:
            x = x.expand(B, n)
        return x.contiguous()

    def forward(self, poses, shapes, Rh=None, Th=None, expression=None, return_verts=True, **kw):
        if poses.dim() != 2 or poses.shape[1] not in (self.NUM_POSES, 3 * self.J):
            raise ValueError(f"SMPLlayer: poses must be (B,{self.NUM_POSES}) or (B,{3 * self.J}), got {tuple(poses.shape)}")
        self.model_struct()                   # refuses buffers that are not float32 before anything is launched
        B = poses.shape[0]
        shapes = self._coef(shapes, self.n_shape, B, "shapes")
        if shapes is None:
            raise ValueError("SMPLlayer: shapes is required")
        expression = self._coef(expression, self.n_expr, B, "expression") if self.n_expr > 0 else None
        for name, t in (("Rh", Rh), ("Th", Th)):
            if t is not None and tuple(t.shape) != (B, 3):
                raise ValueError(f"SMPLlayer: {name} must be (B,3), got {tuple(t.shape)}")
        Rh = None if Rh is None else Rh.float().contiguous()
        Th = None if Th is None else Th.float().contiguous()
        verts, T, A, bs = _BodyModelFn.apply(self, poses.float().contiguous(), shapes, expression, Rh, Th)
        if not return_verts:
            verts = torch.matmul(self.keypoint_regressor(verts.device), verts)
        return verts, T, A, bs

    def keypoint_regressor(self, device):
        if self._kp_regressor is None or self._kp_regressor.device != torch.device(device):
            if self.regressor_path is None:
                reg = self.J_regressor
            else:
                reg = torch.from_numpy(load_regressor(self.regressor_path, self.V))
            self._kp_regressor = reg.to(device=device, dtype=torch.float32)
        return self._kp_regressor


def load_regressor(path, V):
    """(K,V) float32 keypoint regressor from .npy (dense) or .txt (`row col value` triplets, optional `# K V` header)."""
    if path.endswith(".npy"):
        return np.asarray(np.load(path), dtype=np.float32)
    K = None
    trip = []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if not line:
                continue
            if line.startswith("#"):
                vals = line[1:].split()
                if len(vals) >= 2:
                    K, V = int(vals[0]), int(vals[1])
                continue
            r, c, v = line.split()[:3]
            trip.append((int(r), int(c), float(v)))
    t = np.asarray(trip, dtype=np.float64).reshape(-1, 3)
    K = K if K is not None else int(t[:, 0].max()) + 1
    reg = np.zeros((K, V), dtype=np.float32)
    reg[t[:, 0].astype(np.int64), t[:, 1].astype(np.int64)] = t[:, 2]
    return reg


class _BodyModelFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, layer, poses, shapes, expr, Rh, Th):
        require_cuda(poses, shapes, expr, Rh, Th, layer.v_template)
        B, dev = poses.shape[0], poses.device
        V, J = layer.V, layer.J
        verts = torch.empty((B, V, 3), dtype=torch.float32, device=dev)
        T = torch.empty((B, V, 4, 4), dtype=torch.float32, device=dev)
        A = torch.empty((B, J, 4, 4), dtype=torch.float32, device=dev)
        bs = torch.empty((B, V, 3), dtype=torch.float32, device=dev)
        saved = torch.empty((B, _lib.body_saved_floats(J)), dtype=torch.float32, device=dev)
        fb, _ = layer.scratch_bytes(B)
        scratch = torch.empty(max(fb, 1), dtype=torch.uint8, device=dev)
        check(_lib.lib().d3ga_body_model_fwd(ctypes.byref(layer.model_struct()), B, poses.shape[1], dptr(poses), dptr(shapes),
                                            dptr(expr), dptr(Rh), dptr(Th), dptr(verts), dptr(T), dptr(A), dptr(bs),
                                            dptr(saved), dptr(scratch), fb, stream_handle()), "d3ga_body_model_fwd")
        ctx.layer, ctx.pw, ctx.has_expr, ctx.has_Rh, ctx.has_Th = layer, poses.shape[1], expr is not None, Rh is not None, Th is not None
        ctx.save_for_backward(saved, T, bs)
        return verts, T, A, bs

    @staticmethod
    def backward(ctx, g_verts, g_T, g_A, g_bs):
        saved, T, bs = ctx.saved_tensors
        layer = ctx.layer
        B, dev = T.shape[0], T.device
        need = ctx.needs_input_grad
        g_verts, g_A, g_bs = (None if g is None else g.float().contiguous() for g in (g_verts, g_A, g_bs))
        g_T = f32c16(g_T)                     # read as float4 rows
        gp = torch.empty((B, ctx.pw), dtype=torch.float32, device=dev) if need[1] else None
        gs = torch.empty((B, layer.n_shape), dtype=torch.float32, device=dev) if need[2] else None
        ge = torch.empty((B, layer.n_expr), dtype=torch.float32, device=dev) if (need[3] and ctx.has_expr) else None
        gR = torch.empty((B, 3), dtype=torch.float32, device=dev) if (need[4] and ctx.has_Rh) else None
        gT = torch.empty((B, 3), dtype=torch.float32, device=dev) if (need[5] and ctx.has_Th) else None
        _, bb = layer.scratch_bytes(B)
        scratch = torch.empty(max(bb, 1), dtype=torch.uint8, device=dev)
        check(_lib.lib().d3ga_body_model_bwd(ctypes.byref(layer.model_struct()), B, ctx.pw, dptr(saved), dptr(T), dptr(bs),
                                            dptr(g_verts), dptr(g_T), dptr(g_A), dptr(g_bs), dptr(gp), dptr(gs), dptr(ge),
                                            dptr(gR), dptr(gT), dptr(scratch), bb, stream_handle()), "d3ga_body_model_bwd")
        return None, gp, gs, ge, gR, gT
