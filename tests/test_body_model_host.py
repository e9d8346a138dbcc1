"""CPU checks of the SMPL / SMPL-X body model (d3ga_amd/body_model.py): the model-file loader, the error for missing or
chumpy files, the pose-count and buffer shapes, the kernel layouts against the dense float64 products, and known answers
of the float64 oracle (tests/smplx_ref.py) the GPU tests compare with.  Synthetic model files (d3ga_amd.synthetic)."""
import math
import os
import pickle
import sys
import types

import numpy as np
import pytest
import torch

from d3ga_amd import synthetic as syn
from smplx_ref import RefSMPL

V_SMALL = 600          # SMPL-X joints and coefficient counts, fewer vertices: the loader / layout checks run fast


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    d = tmp_path_factory.mktemp("smplx_small")
    data = syn.smpl_model_data("smplx", seed=1, V=V_SMALL)
    paths = {
        "pkl": syn.write_smpl_model(str(d / "dense.pkl"), data),
        "pkl_sparse": syn.write_smpl_model(str(d / "sparse.pkl"), data, sparse_regressor=True),
        "npz": syn.write_smpl_model(str(d / "model.npz"), data),
    }
    gdir = d / "models"
    gdir.mkdir()
    syn.write_smpl_model(str(gdir / "SMPLX_NEUTRAL.pkl"), data)
    syn.write_smpl_model(str(gdir / "SMPL_NEUTRAL.npz"), syn.smpl_model_data("smpl", seed=2, V=400))
    paths["dir"] = str(gdir)
    return data, paths


def _layer(path, **kw):
    from d3ga_amd.body_model import SMPLlayer
    return SMPLlayer(path, model_type=kw.pop("model_type", "smplx"), gender="neutral", use_joints=True, regressor_path=None, **kw)


@pytest.mark.parametrize("kind", ["pkl", "pkl_sparse", "npz", "dir"])
def test_loader_accepts_every_file_form(small, kind):
    data, paths = small
    L = _layer(paths[kind])
    assert L.NUM_POSES == 87 and L.J == 55 and L.V == V_SMALL
    assert L.faces_tensor.dtype == torch.long and tuple(L.faces_tensor.shape) == data["f"].shape
    assert tuple(L.v_template.shape) == (V_SMALL, 3) and tuple(L.weights.shape) == (V_SMALL, 55)
    assert tuple(L.J_regressor.shape) == (55, V_SMALL)
    assert np.abs(L.J_regressor.double().numpy() - data["J_regressor"]).max() < 1e-7
    assert np.abs(L.v_template.double().numpy() - data["v_template"]).max() < 1e-6
    names = dict(L.named_buffers())
    for k in ("faces_tensor", "v_template", "weights", "J_regressor", "bm_dirs"):
        assert k in names                         # buffers: .cuda() moves them


def test_smpl_model_type(small):
    _, paths = small
    L = _layer(paths["dir"], model_type="smpl")
    assert L.NUM_POSES == 72 and L.J == 24 and L.n_expr == 0 and L.V == 400
    assert tuple(L.weights.shape) == (400, 24) and tuple(L.J_regressor.shape) == (24, 400)


def test_missing_model_file_is_file_not_found_and_not_implemented(tmp_path):
    from d3ga_amd.body_model import SMPLlayer
    missing = str(tmp_path / "nowhere")
    with pytest.raises(FileNotFoundError) as ei:
        SMPLlayer(missing, model_type="smplx", gender="neutral")
    assert isinstance(ei.value, NotImplementedError)
    msg = str(ei.value)
    assert "SMPL-X" in msg and missing in msg and "SMPLX_NEUTRAL.pkl" in msg
    with pytest.raises(NotImplementedError, match="SMPL-X"):
        SMPLlayer(str(tmp_path / "model.pkl"))
    # the compat path and the earlier import location serve the same class
    import d3ga_amd.cage_deform as C
    from d3ga_amd.body_model import SMPLlayer as S
    assert C.SMPLlayer is S


def test_chumpy_pickle_is_refused_clearly(tmp_path):
    mod, sub = types.ModuleType("chumpy"), types.ModuleType("chumpy.ch")

    class Ch:
        def __init__(self, x):
            self.x = x

    Ch.__module__, Ch.__qualname__ = "chumpy.ch", "Ch"
    sub.Ch = Ch
    mod.ch = sub
    sys.modules["chumpy"], sys.modules["chumpy.ch"] = mod, sub
    try:
        data = syn.smpl_model_data("smpl", seed=3, V=200)
        data["shapedirs"] = Ch(data["shapedirs"])
        p = str(tmp_path / "SMPL_NEUTRAL.pkl")
        with open(p, "wb") as f:
            pickle.dump(data, f, protocol=2)
    finally:
        del sys.modules["chumpy"], sys.modules["chumpy.ch"]
    with pytest.raises(ValueError, match="chumpy"):
        _layer(p, model_type="smpl")


def test_layouts_reproduce_dense_products(small):
    data, paths = small
    L = _layer(paths["pkl_sparse"])
    V, J, NS = L.V, L.J, L.n_shape + L.n_expr
    vt = data["v_template"]
    sd = data["shapedirs"]
    se = np.concatenate([sd[:, :, :10], sd[:, :, 300:310]], axis=2)        # S = 400: expression at 300:310
    pd = np.asarray(data["posedirs"], np.float64)
    dirs = L.bm_dirs.double().numpy()
    assert dirs.shape == (NS + 9 * (J - 1), L.ld) and L.ld % 2048 == 0 and L.ld >= 3 * V
    assert np.abs(dirs[:, 3 * V:]).max() == 0
    rng = np.random.default_rng(0)
    c, pf = rng.normal(size=NS), rng.normal(size=9 * (J - 1))
    want = np.einsum("vcs,s->vc", se, c) + np.einsum("vcp,p->vc", pd, pf)
    got = (dirs[:, :3 * V].T @ np.concatenate([c, pf])).reshape(V, 3)
    assert np.abs(got - want).max() < 1e-6 * np.abs(want).max()
    Jreg = data["J_regressor"]
    assert np.abs(L.bm_J0.double().numpy() - Jreg @ vt).max() < 1e-6
    Jd = L.bm_Jdirs.double().numpy()
    assert np.abs(np.einsum("sjc,s->jc", Jd, c) - Jreg @ np.einsum("vcs,s->vc", se, c)).max() < 1e-6
    # CSR by vertex and by joint: every nonzero, nothing else
    W = data["weights"]
    ptr, jj, ww = L.bm_w_ptr.numpy(), L.bm_w_joint.numpy(), L.bm_w_val.double().numpy()
    Wr = np.zeros_like(W)
    for v in range(V):
        Wr[v, jj[ptr[v]:ptr[v + 1]]] = ww[ptr[v]:ptr[v + 1]]
    assert np.abs(Wr - W).max() < 1e-7 and len(jj) == np.count_nonzero(W)
    tp, tv, tw = L.bm_wt_ptr.numpy(), L.bm_wt_vert.numpy(), L.bm_wt_val.double().numpy()
    Wc = np.zeros_like(W)
    for j in range(J):
        seg = tv[tp[j]:tp[j + 1]]
        assert np.all(np.diff(seg) > 0)
        Wc[seg, j] = tw[tp[j]:tp[j + 1]]
    assert np.abs(Wc - W).max() < 1e-7
    # levels: a joint's parent sits in an earlier level; children lists match parents
    parents = L.bm_parents.numpy()
    lp, lj = L.bm_level_ptr.numpy(), L.bm_level_joint.numpy()
    level = np.empty(J, np.int64)
    for lv in range(len(lp) - 1):
        level[lj[lp[lv]:lp[lv + 1]]] = lv
    assert sorted(lj.tolist()) == list(range(J)) and parents[0] == -1
    assert all(level[j] == level[parents[j]] + 1 for j in range(1, J))
    cp, cj = L.bm_child_ptr.numpy(), L.bm_child_joint.numpy()
    for j in range(J):
        assert sorted(cj[cp[j]:cp[j + 1]].tolist()) == [k for k in range(J) if parents[k] == j]
    # hand PCA: 6 components, flat mean
    assert tuple(L.bm_hand_comps.shape) == (2, 6, 45)
    assert np.abs(L.bm_hand_comps[0].double().numpy() - data["hands_componentsl"][:6]).max() < 1e-6
    assert float(L.bm_hand_mean.abs().max()) == 0.0


def test_oracle_rest_pose_is_identity(small):
    data, _ = small
    ref = RefSMPL(data)
    B = 2
    v, T, A, bs = ref(torch.zeros(B, 87, dtype=torch.float64), torch.zeros(1, 10, dtype=torch.float64))
    eye = torch.eye(4, dtype=torch.float64)
    assert (A - eye).abs().max() < 1e-14 and (T - eye).abs().max() < 1e-14
    assert (v - torch.from_numpy(data["v_template"])).abs().max() < 1e-14 and bs.abs().max() < 1e-14


def test_oracle_one_joint_moves_only_its_subtree(small):
    data = dict(small[0])
    data["posedirs"] = np.zeros_like(data["posedirs"])            # pose blend shapes move every vertex: off for this check
    ref = RefSMPL(data)
    parents = ref.parents
    j = next(k for k in range(1, 55) if sum(1 for q in parents if q == k) > 0 and k < 22)
    sub = {j}
    for k in range(55):
        if parents[k] in sub:
            sub.add(k)
    poses = torch.zeros(1, 165, dtype=torch.float64)
    poses[0, 3 * j:3 * j + 3] = torch.tensor([0.4, -0.3, 0.5])
    v, *_ = ref(poses, torch.zeros(1, 10, dtype=torch.float64))
    moved = ((v[0] - torch.from_numpy(data["v_template"])).norm(dim=1) > 1e-12).numpy()
    touched = (data["weights"][:, sorted(sub)] > 0).any(axis=1)
    assert moved.any() and not np.any(moved & ~touched)


def test_oracle_unpose_recovers_the_template(small):
    """Smplman.create_body_model (lib/smplman.py:96-100): unpose(T (v_t + bs)) - bs = v_t."""
    data, _ = small
    ref = RefSMPL(data)
    g = torch.Generator().manual_seed(4)
    poses = torch.zeros(1, 87, dtype=torch.float64)
    poses[:, 5], poses[:, 8] = math.pi / 6, -math.pi / 6        # the star pose (lib/smplman.py:126-127)
    poses[:, 9:66] += 0.2 * torch.randn(1, 57, generator=g, dtype=torch.float64)
    shapes = torch.randn(1, 10, generator=g, dtype=torch.float64)
    v, T, A, bs = ref(poses, shapes, expression=torch.randn(1, 10, generator=g, dtype=torch.float64))
    homo = torch.cat([v, torch.ones_like(v[..., :1])], dim=-1)[..., None]
    vtn = (torch.inverse(T) @ homo)[..., :3, 0] - bs
    assert (vtn - torch.from_numpy(data["v_template"])).abs().max() < 1e-12


def test_compact_and_full_pose_layouts_agree_in_the_oracle(small):
    data, _ = small
    ref = RefSMPL(data)
    g = torch.Generator().manual_seed(5)
    p87 = 0.3 * torch.randn(2, 87, generator=g, dtype=torch.float64)
    full = ref.full_pose(p87)
    assert full.shape == (2, 165)
    assert torch.equal(full[:, :66], p87[:, :66]) and torch.equal(full[:, 66:75], p87[:, 78:87])
    hl = p87[:, 66:72] @ torch.from_numpy(data["hands_componentsl"][:6])
    assert (full[:, 75:120] - hl).abs().max() < 1e-14
    a = ref(p87, torch.zeros(1, 10, dtype=torch.float64))
    b = ref(full, torch.zeros(1, 10, dtype=torch.float64))
    for x, y in zip(a, b):
        assert (x - y).abs().max() < 1e-14


# ---------------------------------------------------------------------------------------------------------------------
# refusals: configurations the kernels cannot serve are turned away before anything is launched
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [46, 50, -1])
def test_hand_pca_outside_0_to_45_is_refused(small, n):
    """hands_components is (45, 45): more components would make the kernels read past hand_comps."""
    _, paths = small
    with pytest.raises(ValueError, match="num_pca_comps"):
        _layer(paths["pkl"], num_pca_comps=n)


def test_45_hand_components_keep_the_full_pose_width(small):
    _, paths = small
    L = _layer(paths["pkl"], num_pca_comps=45)
    assert L.n_hand_pca == 45 and L.NUM_POSES == 165 == 3 * L.J


@pytest.mark.parametrize("J", [1, 65])
def test_joint_count_outside_2_to_64_is_refused(tmp_path, J):
    """J = 65 is beyond D3GA_BODY_MAX_JOINTS (the kernels' LDS tables); J = 1 has no posed joint (no pose blend shapes):
    a rigid body is the global Rh / Th of any model."""
    p = syn.write_smpl_model(str(tmp_path / "m.npz"), syn.smpl_model_data("smpl", seed=3, V=40, J=J))
    with pytest.raises(ValueError, match=f"{J} joint"):
        _layer(p, model_type="smpl")


def test_converted_layer_is_refused_before_any_launch(small):
    """.double() / .half() convert the float buffers; the kernels read float32, so the layer refuses them (on the CPU too,
    i.e. before the device check and any launch)."""
    _, paths = small
    for conv in (lambda m: m.double(), lambda m: m.half()):
        L = conv(_layer(paths["pkl"]))
        with pytest.raises(TypeError, match="float32"):
            L.model_struct()
        with pytest.raises(TypeError, match="float32"):
            L(poses=torch.zeros(1, 87), shapes=torch.zeros(1, 10))
    L = _layer(paths["pkl"]).double().float()         # back to float32: accepted again
    assert L.model_struct().n_hand_pca == 6


def test_c_abi_refuses_more_than_45_hand_components(small):
    """body_check, reached through ctypes with no device: n_hand_pca > 45 and J < 2 are D3GA_E_SIZE for C callers too, and
    a 165-wide pose with 45 components is the (accepted) full layout -- the call then stops at its NULL outputs."""
    import ctypes
    from d3ga_amd import _lib
    _, paths = small
    L = _layer(paths["pkl"], num_pca_comps=45)
    lib = _lib.lib()

    def fwd(s, pw):
        return lib.d3ga_body_model_fwd(ctypes.byref(s), 1, pw, None, None, None, None, None, None, None, None, None, None,
                                       None, 0, None)

    def bwd(s, pw):
        return lib.d3ga_body_model_bwd(ctypes.byref(s), 1, pw, None, None, None, None, None, None, None, None, None, None,
                                       None, None, None, 0, None)

    s = L.model_struct()
    assert fwd(s, 165) == -1 and bwd(s, 165) == -1            # D3GA_E_NULL: past the layout checks
    for field, value in (("n_hand_pca", 46), ("n_hand_pca", 90), ("J", 1)):
        t = _lib.BodyModel.from_buffer_copy(s)
        setattr(t, field, value)
        assert fwd(t, 165) == -2 and bwd(t, 165) == -2, (field, value)        # D3GA_E_SIZE
