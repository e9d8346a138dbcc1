"""CPU-side checks of the Goliath skeleton (d3ga_amd/skeleton_model.py, csrc/skeleton_math.h): the float64 oracle
(tests/goliath_ref.py) against the reference's own recorded values and autograd gradients (tests/golden/skeleton_cases.npz),
the per-joint math header built for the host against that oracle, the CSR / CSC of the parameter transform, the refusals of
the layer, the state-dict names, the declared entry points, and the float32 margin of the GPU fuzz ranges.

Bars: values |a - b| <= 1e-5 max|b|; gradients util.elementwise_excess <= 1."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import goliath_ref as gr
from conftest import ROOT
from util import elementwise_excess

FWD_BAR = 1e-5


def fwd_err(a, b):
    b = np.asarray(b, np.float64)
    return float(np.abs(np.asarray(a, np.float64).reshape(b.shape) - b).max() / (np.abs(b).max() + 1e-300))


def golden_rig(z, normalise=False):
    rot = z["joint_rotation"].astype(np.float64)
    if normalise:
        rot = rot / np.linalg.norm(rot, axis=1, keepdims=True)
    return gr.Rig(z["transform"], z["transform_offsets"], z["joint_offset"], rot, z["parents"], z["skin_indices"], z["skin_weights"])


def golden_module(z):
    from d3ga_amd.skeleton_model import LBSModule
    return LBSModule(gr.rig_json(z["joint_offset"], z["joint_rotation"], z["parents"], z["skin_indices"], z["skin_weights"], z["rest"]),
                     gr.rig_config(z["transform"], z["transform_offsets"], z["poses"].shape[1], z["scales"].shape[1]),
                     z["template"], z["lbs_scale"], z["global_scaling"])


def oracle_on_golden(z, normalise=False):
    rig = golden_rig(z, normalise)
    d = torch.float64
    poses = torch.tensor(z["poses"], dtype=d, requires_grad=True)
    scales = torch.tensor(z["scales"], dtype=d, requires_grad=True)
    verts = torch.tensor(z["verts"], dtype=d, requires_grad=True)
    out = {}
    out["param"] = gr.skeleton_params(rig.transform, rig.offsets, poses, scales)
    out["bind_state"] = rig.bind
    out["states"] = rig.states(poses, scales)
    out["mat"] = gr.matrices(rig.bind, out["states"])
    out["out"] = rig.forward(poses, scales, verts)
    gp, gs, gv = torch.autograd.grad((out["out"] * torch.tensor(z["grad_out"], dtype=d)).sum(), [poses, scales, verts])
    t_root, R_root = rig.root(poses)
    out["t_root"], out["R_root"] = t_root, R_root
    (gpr,) = torch.autograd.grad((t_root * torch.tensor(z["grad_t_root"], dtype=d)).sum()
                                 + (R_root * torch.tensor(z["grad_R_root"], dtype=d)).sum(), [poses])
    B = poses.shape[0]
    out["posed"] = rig.forward(poses, torch.tensor(z["lbs_scale"], dtype=d).expand(B, -1),
                               torch.tensor(z["template"], dtype=d)[None]) * torch.tensor(z["global_scaling"], dtype=d)
    grads = dict(grad_poses=gp, grad_scales=gs, grad_verts=gv, grad_poses_root=gpr)
    return {k: v.detach().numpy() for k, v in out.items()}, {k: v.numpy() for k, v in grads.items()}


def test_oracle_matches_the_reference_on_every_captured_quantity(golden):
    z = golden("skeleton_cases.npz")
    assert abs(np.linalg.norm(z["joint_rotation"][3]) - 1.001) < 1e-5 and abs(np.linalg.norm(z["joint_rotation"][11]) - 0.999) < 1e-5
    vals, grads = oracle_on_golden(z)
    for k, v in vals.items():
        e = fwd_err(v, z[k])
        print(f"[skeleton golden] {k}: {e:.2e} of max|ref|")
        assert e <= FWD_BAR, (k, e)
    for k, v in grads.items():
        e = elementwise_excess(z[k], v)          # the reference's float32 gradient against the float64 oracle
        print(f"[skeleton golden] {k}: excess {e:.3f}")
        assert e <= 1.0, (k, e)


def test_golden_tells_as_given_from_normalised_first(golden):
    """The two pre-rotations of norm 1 +- 1e-3 are among the checked joints: an oracle that normalises them first misses the bar."""
    z = golden("skeleton_cases.npz")
    vals, _ = oracle_on_golden(z, normalise=True)
    assert fwd_err(vals["mat"], z["mat"]) > 10 * FWD_BAR
    assert fwd_err(vals["out"], z["out"]) > 10 * FWD_BAR


# ----------------------------------------------------------------------------------------------------------------------
# the math header on the host
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def skmath():
    src = os.path.join(ROOT, "tests", "hostcheck", "skeleton_check.cpp")
    hdr = os.path.join(ROOT, "d3ga_amd", "csrc", "skeleton_math.h")
    out_dir = os.path.join(ROOT, "tests", "hostcheck", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libskeleton_check.so")
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in (src, hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", so])
    return ctypes.CDLL(so)


def _call(fn, ins, out_sizes):
    fp = ctypes.POINTER(ctypes.c_float)
    ins = [np.ascontiguousarray(a, dtype=np.float32) for a in ins]
    outs = [np.full(n, np.nan, dtype=np.float32) for n in out_sizes]
    fn(*[a.ctypes.data_as(fp) for a in ins + outs])
    return outs


def _angle_sets():
    rng = np.random.default_rng(5)
    A = np.asarray(gr.EDGE_ANGLES)
    sets = [np.array([a, b, c]) for a in (0.0, 1e-6, 6.0) for b in (0.0, -1e-6, -6.0) for c in (0.0, 1e-6, 4.5)]
    sets += [A[rng.integers(0, len(A), 3)] * rng.choice([-1.0, 1.0], 3) for _ in range(60)]
    return sets


def _t(a):
    return torch.tensor(np.asarray(a, dtype=np.float32).astype(np.float64), requires_grad=True)


def _check(name, got_fwd, ref_fwd, got_bwd, ref_bwd):
    for g, r in zip(got_fwd, ref_fwd):
        e = fwd_err(g, r.detach().numpy())
        assert e <= FWD_BAR, (name, "forward", e)
    for g, r in zip(got_bwd, ref_bwd):
        e = elementwise_excess(g, r.numpy())
        assert e <= 1.0, (name, "backward", e)


def test_math_header_on_the_host_against_float64_autograd(skmath):
    rng = np.random.default_rng(7)

    def quat(unit=False):
        q = rng.normal(size=4)
        return q / np.linalg.norm(q) * (1.0 if unit else rng.uniform(0.8, 1.25))

    def state():
        return np.concatenate([rng.normal(size=3), quat(), [2.0 ** rng.uniform(-1, 1)]])

    for r in _angle_sets():
        p = np.concatenate([rng.normal(size=3), r, [rng.uniform(-1.0, 1.0)]])
        off, pre = rng.normal(size=3), quat()
        a, b, v = quat(), quat(), rng.normal(size=3)
        P, l, bind, S = state(), state(), state(), state()
        g4, g3, g8, g12 = rng.normal(size=4), rng.normal(size=3), rng.normal(size=8), rng.normal(size=12)

        ta, tb = _t(a), _t(b)
        o = gr.qmul(ta, tb)
        _check("qmul", _call(skmath.sk_qmul, [a, b], [4]), [o], _call(skmath.sk_qmul_bwd, [a, b, g4], [4, 4]),
               torch.autograd.grad((o * _t(g4).detach()).sum(), [ta, tb]))

        tq, tv = _t(a), _t(v)
        o = gr.qrot(tq, tv)
        _check("qrot", _call(skmath.sk_qrot, [a, v], [3]), [o], _call(skmath.sk_qrot_bwd, [a, v, g3], [4, 3]),
               torch.autograd.grad((o * _t(g3).detach()).sum(), [tq, tv]))

        tr = _t(r)
        o = gr.euler_quat(tr)
        _check("euler_quat", _call(skmath.sk_euler_quat, [r], [4]), [o], _call(skmath.sk_euler_quat_bwd, [r, g4], [3]),
               torch.autograd.grad((o * _t(g4).detach()).sum(), [tr]))

        tp = _t(p)
        o = gr.local_states(tp[None], _t(off).detach()[None], _t(pre).detach()[None])[0, 0]
        (lf,) = _call(skmath.sk_local_state, [p, off, pre], [8])
        _check("local_state", [lf], [o], _call(skmath.sk_local_state_bwd, [p, pre, lf, g8], [7]),
               torch.autograd.grad((o * _t(g8).detach()).sum(), [tp]))

        tP, tl = _t(P), _t(l)
        o = gr.chain(tP, tl)
        _check("chain_step", _call(skmath.sk_chain_step, [P, l], [8]), [o], _call(skmath.sk_chain_step_bwd, [P, l, g8], [8, 8]),
               torch.autograd.grad((o * _t(g8).detach()).sum(), [tP, tl]))

        tS = _t(S)
        o = gr.matrices(_t(bind).detach()[None], tS[None, None])[0, 0]
        _check("joint_matrix", _call(skmath.sk_joint_matrix, [bind, S], [12]), [o.reshape(-1)],
               _call(skmath.sk_joint_matrix_bwd, [bind, S, g12], [8]),
               torch.autograd.grad((o.reshape(-1) * _t(g12).detach()).sum(), [tS]))


# ----------------------------------------------------------------------------------------------------------------------
# parameter-transform tables
# ----------------------------------------------------------------------------------------------------------------------
def test_transform_tables_reproduce_the_dense_product_exactly():
    from d3ga_amd.skeleton_model import csc_apply_t, csr_apply, transform_tables
    rng = np.random.default_rng(3)
    for R, P in ((14, 5), (21, 1), (7 * 30, 33)):
        T = rng.normal(size=(R, P)) * (rng.random((R, P)) < 0.1)
        T[R // 2] = 0.0                                   # an empty row
        T[:, P - 1] = 0.0                                 # a parameter no joint reads
        tab = transform_tables(T)
        assert tab["csr_ptr"][R // 2] == tab["csr_ptr"][R // 2 + 1] and tab["csc_ptr"][P - 1] == tab["csc_ptr"][P]
        assert len(tab["csr_val"]) == np.count_nonzero(T) == len(tab["csc_val"])
        for r in range(R):
            assert np.all(np.diff(tab["csr_col"][tab["csr_ptr"][r]:tab["csr_ptr"][r + 1]]) > 0)
        for p in range(P):
            assert np.all(np.diff(tab["csc_row"][tab["csc_ptr"][p]:tab["csc_ptr"][p + 1]]) > 0)
        x, g = rng.normal(size=P), rng.normal(size=R)
        dense = np.zeros(R)
        for c in range(P):                                # the dense product in the same (ascending) order: zeros add nothing
            dense = dense + T[:, c] * x[c]
        dense_t = np.zeros(P)
        for r in range(R):
            dense_t = dense_t + T[r] * g[r]
        assert np.array_equal(csr_apply(tab, x), dense)
        assert np.array_equal(csc_apply_t(tab, g), dense_t)


# ----------------------------------------------------------------------------------------------------------------------
# the layer
# ----------------------------------------------------------------------------------------------------------------------
def test_state_dict_keys_are_the_reference_modules(golden):
    z = golden("skeleton_cases.npz")
    m = golden_module(z)
    assert list(m.state_dict().keys()) == [str(k) for k in z["state_dict_keys"]]
    # the bind state the constructor solves in float32 torch is the reference's
    assert fwd_err(m.lbs_fn.bind_state.numpy(), z["bind_state"]) <= FWD_BAR
    assert m.lbs_fn.skin_indices.dtype == torch.int64 and tuple(m.lbs_fn.skin_weights.shape) == (200, 8)
    np.testing.assert_array_equal(m.lbs_fn.skin_weights.numpy().sum(1) > 0.99, True)
    m.load_state_dict({k: v.clone() for k, v in m.state_dict().items()}, strict=True)


def test_scale_file_becomes_a_one_row_buffer(golden, tmp_path):
    """`scale_path`: a text file of scale parameters, one set per line (or a single line); the buffer `scale` is its first set as
    (1, n) float32 and is part of the state dict, after the reference's other buffers of the module."""
    from d3ga_amd.skeleton_model import LinearBlendSkinning
    z = golden("skeleton_cases.npz")
    model = gr.rig_json(z["joint_offset"], z["joint_rotation"], z["parents"], z["skin_indices"], z["skin_weights"], z["rest"])
    cfg = gr.rig_config(z["transform"], z["transform_offsets"], 10, 4)
    rows = np.asarray([[0.25, -0.5, 0.125, 1.5], [9.0, 9.0, 9.0, 9.0]])
    for name, content in (("one.txt", rows[:1]), ("flat.txt", rows[0]), ("two.txt", rows)):
        path = tmp_path / name
        np.savetxt(path, content)
        m = LinearBlendSkinning(model, cfg, scale_path=str(path))
        assert m.scale.dtype == torch.float32 and tuple(m.scale.shape) == (1, 4), name
        np.testing.assert_array_equal(m.scale.numpy(), rows[:1].astype(np.float32))
        keys = list(m.state_dict().keys())
        assert keys.index("scale") == keys.index("joints_weights") + 1 and keys[-1] == "param_transform.transform"
    assert "scale" not in LinearBlendSkinning(model, cfg).state_dict()


def test_several_roots_and_two_joints():
    """The tree tables with more than one root, and the smallest rig: levels hold every joint once, a parent in an earlier level,
    children ascending under their parent."""
    from d3ga_amd.body_model import tree_tables
    from d3ga_amd.skeleton_model import check_parents
    for par in ([-1, -1], [-1, 0], [-1, 0, -1, 2, 2, 0, -1, 3]):
        check_parents(np.asarray(par))
        lp, lj, cp, cj, depth = tree_tables(np.asarray(par, dtype=np.int64))
        assert sorted(lj.tolist()) == list(range(len(par))) and lp[0] == 0 and lp[-1] == len(par)
        level_of = {int(j): L for L in range(len(lp) - 1) for j in lj[lp[L]:lp[L + 1]]}
        for j, p in enumerate(par):
            assert level_of[j] == (0 if p < 0 else level_of[p] + 1) == depth[j]
            assert cj[cp[j]:cp[j + 1]].tolist() == [c for c in range(len(par)) if par[c] == j]
        assert len(cj) == sum(p >= 0 for p in par)
    rng = np.random.default_rng(2)
    rig = gr.random_rig(rng, 40, 6, 2, kind="forest")
    assert (rig.parents < 0).sum() > 1


def test_refusals(golden):
    from d3ga_amd import D3GAError
    from d3ga_amd import skeleton_model as sm
    z = golden("skeleton_cases.npz")
    J = len(z["parents"])
    off, rot = torch.tensor(z["joint_offset"]), torch.tensor(z["joint_rotation"])
    par = z["parents"].astype(np.int64).copy()
    par[4], par[9] = 9, 4                                               # joint 4 hangs on the later joint 9
    with pytest.raises(ValueError, match="joint 4 "):
        sm.solve_skeleton_state(torch.zeros(1, 7 * J), off, rot, torch.tensor(par))
    with pytest.raises(ValueError, match="joint 4 "):
        sm.LinearBlendSkinning(gr.rig_json(z["joint_offset"], z["joint_rotation"], par, z["skin_indices"], z["skin_weights"], z["rest"]),
                               gr.rig_config(z["transform"], z["transform_offsets"], 10, 4))
    par = z["parents"].astype(np.int64).copy()
    par[6] = 6
    with pytest.raises(ValueError, match="joint 6 is its own parent"):
        sm.solve_skeleton_state(torch.zeros(1, 7 * J), off, rot, torch.tensor(par))
    m = golden_module(z)
    motion = torch.zeros(2, 10)
    with pytest.raises(ValueError, match="parameters"):
        m.lbs_fn(torch.zeros(2, 15), torch.zeros(2, 4))                  # 19 parameters for a model of 14
    with pytest.raises(ValueError, match="scales"):
        m.lbs_fn(motion, torch.zeros(2, 3))
    with pytest.raises(D3GAError, match="GPU only"):
        m.pose(motion)                                                    # a CPU module
    with pytest.raises(D3GAError, match="GPU only"):
        sm.states_to_matrix(m.lbs_fn.bind_state, torch.zeros(2, J, 8))
    with pytest.raises(TypeError, match="float32"):
        golden_module(z).double().pose(motion.double())
    with pytest.raises(TypeError, match="float32"):
        golden_module(z).half().lbs_fn.compute_root_rigid_transform(motion)
    with pytest.raises(TypeError, match="float32"):
        sm.goliath_cage(golden_module(z).double(), motion)


def test_setup_paths_in_plain_torch(golden):
    """unpose inverts the skinning; compute_joints_weights is the dense form of the sparse tables (CPU, no kernels)."""
    z = golden("skeleton_cases.npz")
    m = golden_module(z)
    lbs = m.lbs_fn
    poses, scales, verts = torch.tensor(z["poses"]), torch.tensor(z["scales"]), torch.tensor(z["verts"])
    back = lbs.unpose(poses, scales, torch.tensor(z["out"]))
    assert fwd_err(back.numpy(), verts.numpy()) <= 1e-4
    W = lbs.compute_joints_weights()
    # (the synthetic rig repeats joints within a row: the scatter keeps one of the repeated weights, as the reference's does)
    assert tuple(W.shape) == (24, 200) and float(W.min()) >= 0 and float(W.sum(0).max()) <= 1 + 1e-5
    v = 17
    assert all(float(W[lbs.skin_indices[v, k], v]) in lbs.skin_weights[v].tolist() for k in range(8))
    rel = lbs.compute_relative_rigid_transforms(poses[:, :6], poses[:, 6:], scales)
    ref = gr.local_states(torch.tensor(z["param"]).double(), torch.tensor(z["joint_offset"]).double(), torch.tensor(z["joint_rotation"]).double())
    assert fwd_err(rel.numpy(), ref[..., :7].numpy()) <= FWD_BAR


def test_header_declares_the_skeleton_entry_points():
    src = open(os.path.join(ROOT, "include", "d3ga.h")).read()
    assert int(re.search(r"#define\s+D3GA_VERSION\s+(\d+)", src).group(1)) == 112
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    from d3ga_amd import _lib
    for name in ("d3ga_skeleton_check", "d3ga_skeleton_fwd", "d3ga_skeleton_bwd", "d3ga_skeleton_mats_fwd", "d3ga_skeleton_mats_bwd"):
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in _lib.EXPORTS
    assert _lib.ABI_VERSION == 112
    assert int(re.search(r"#define\s+D3GA_SKEL_MAX_JOINTS\s+(\d+)", src).group(1)) == _lib.SKEL_MAX_JOINTS >= 512
    assert int(re.search(r"#define\s+D3GA_SKEL_SAVED_FLOATS\s+(\d+)", src).group(1)) == _lib.SKEL_SAVED_FLOATS


# ----------------------------------------------------------------------------------------------------------------------
# the fuzz ranges of tests/test_gpu_skeleton.py: float32 alone must stay within half of each bar
# ----------------------------------------------------------------------------------------------------------------------
def test_fuzz_ranges_leave_float32_half_of_each_bar():
    """A check of the oracle and of the chosen input ranges, not of the kernels: it needs tests/goliath_ref.py alone."""
    worst_f, worst_g = 0.0, 0.0
    for seed in range(int(os.environ.get("D3GA_SKEL_MARGIN_N", "60"))):
        case = gr.fuzz_case(seed)
        a, b = gr.fuzz_eval(case, torch.float32), gr.fuzz_eval(case, torch.float64)
        f = max(fwd_err(a[k], b[k]) for k in ("states", "mats", "root"))
        g = max(elementwise_excess(a[k], b[k]) for k in ("g_poses", "g_scales") if b[k].size)
        worst_f, worst_g = max(worst_f, f), max(worst_g, g)
        assert f <= 0.5 * FWD_BAR and g <= 0.5, (seed, case["J"], case["kind"], f, g)
        case = gr.free_case(seed)                   # the free functions' cases, same ranges
        a, b = gr.free_eval(case, torch.float32), gr.free_eval(case, torch.float64)
        f = max(fwd_err(a[k], b[k]) for k in ("states", "mats"))
        g = elementwise_excess(a["g_param"], b["g_param"])
        worst_f, worst_g = max(worst_f, f), max(worst_g, g)
        assert f <= 0.5 * FWD_BAR and g <= 0.5, ("free", seed, case["J"], case["kind"], f, g)
    print(f"[skeleton fuzz margin] float32 vs float64 oracle: forward {worst_f / FWD_BAR:.3f} of the bar, gradients {worst_g:.3f}")
