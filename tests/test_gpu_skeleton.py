"""GPU checks of the Goliath skeleton kernels (csrc/skeleton.hip) and their layer (d3ga_amd/skeleton_model.py) against the
float64 oracle (tests/goliath_ref.py) and the reference's recorded values and gradients (tests/golden/skeleton_cases.npz).

Bars: values |a - b| <= 1e-5 max|b|; gradients util.elementwise_excess <= 1.  The fuzz ranges
(goliath_ref.FUZZ_*) leave float32 arithmetic half of each bar (tests/test_skeleton_host.py measures that on the CPU).
D3GA_SKEL_FUZZ_N: number of fuzz cases (default 40; a campaign runs thousands)."""
import os

import numpy as np
import pytest
import torch

import goliath_ref as gr
from test_skeleton_host import FWD_BAR, fwd_err, golden_module, golden_rig
from util import elementwise_excess

pytestmark = pytest.mark.gpu
DEV = "cuda"


def d64(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


def check_vals(name, got, ref):
    e = fwd_err(got.detach().cpu().numpy(), ref.detach().numpy() if torch.is_tensor(ref) else ref)
    print(f"[skeleton] {name}: {e:.2e} of max|ref|")
    assert e <= FWD_BAR, (name, e)


def check_grad(name, got, ref):
    e = elementwise_excess(got.detach().cpu().numpy(), ref.detach().numpy() if torch.is_tensor(ref) else ref)
    print(f"[skeleton] {name}: excess {e:.3f}")
    assert e <= 1.0, (name, e)


def test_golden_rig_against_the_reference(golden):
    """Values and gradients the reference itself recorded, through the drop-in classes and the free functions."""
    from d3ga_amd import skeleton_model as sm
    z = golden("skeleton_cases.npz")
    m = golden_module(z).to(DEV)
    lbs = m.lbs_fn
    poses = torch.tensor(z["poses"], device=DEV, requires_grad=True)
    scales = torch.tensor(z["scales"], device=DEV, requires_grad=True)
    verts = torch.tensor(z["verts"], device=DEV, requires_grad=True)
    param = lbs.param_transform(torch.cat([poses, scales], 1))
    check_vals("param", param, z["param"])
    states = sm.solve_skeleton_state(param, lbs.joint_offset, lbs.joint_rotation, lbs.joint_parents)
    check_vals("states (free function)", states, z["states"])
    check_vals("mat (free function)", sm.states_to_matrix(lbs.bind_state, states), z["mat"])
    check_vals("states (layer)", lbs.compute_rigid_transforms(poses[:, :6], poses[:, 6:], scales), z["states"])
    check_vals("mat (layer)", lbs.compute_rigid_transforms_matrix(poses[:, :6], poses[:, 6:], scales), z["mat"])
    out = lbs(poses, scales, verts)
    check_vals("out", out, z["out"])
    check_vals("skinning", lbs.skinning(lbs.bind_state, verts, states), z["out"])
    gp, gs, gv = torch.autograd.grad((out * torch.tensor(z["grad_out"], device=DEV)).sum(), [poses, scales, verts])
    check_grad("grad_poses", gp, z["grad_poses"])
    check_grad("grad_scales", gs, z["grad_scales"])
    check_grad("grad_verts", gv, z["grad_verts"])
    # the same gradient through the free functions: param -> states -> matrices -> skinning
    out2 = lbs.skinning(lbs.bind_state, verts, states)
    gp2, gs2 = torch.autograd.grad((out2 * torch.tensor(z["grad_out"], device=DEV)).sum(), [poses, scales])
    check_grad("grad_poses (free functions)", gp2, z["grad_poses"])
    check_grad("grad_scales (free functions)", gs2, z["grad_scales"])
    t_root, R_root = lbs.compute_root_rigid_transform(poses)
    check_vals("t_root", t_root, z["t_root"])
    check_vals("R_root", R_root, z["R_root"])
    (gpr,) = torch.autograd.grad((t_root * torch.tensor(z["grad_t_root"], device=DEV)).sum()
                                 + (R_root * torch.tensor(z["grad_R_root"], device=DEV)).sum(), [poses])
    check_grad("grad_poses_root", gpr, z["grad_poses_root"])
    check_vals("posed", m.pose(poses.detach()), z["posed"])
    check_vals("template_pose", m.template_pose(poses.detach()), z["posed"])
    mat, (tr, tt, ts) = sm.states_to_matrix(lbs.bind_state, states.detach(), return_transform=True)
    check_vals("return_transform translation", tt, z["mat"][..., 3])


@pytest.mark.parametrize("B", [1, 3, 20])
def test_parity_with_the_oracle(golden, B):
    """Forward (states, matrices, root, posed vertices, cage) and gradients (motion, scales, template, delta) for B frames."""
    from d3ga_amd.skeleton_model import goliath_cage
    z = golden("skeleton_cases.npz")
    m = golden_module(z).to(DEV)
    lbs, rig = m.lbs_fn, golden_rig(z)
    g = torch.Generator().manual_seed(100 + B)
    NP, NS, V = z["poses"].shape[1], z["scales"].shape[1], z["rest"].shape[0]
    poses64 = (0.8 * torch.randn(B, NP, generator=g, dtype=torch.float64)).float().double().requires_grad_(True)
    scales64 = (0.3 * torch.randn(B, NS, generator=g, dtype=torch.float64)).float().double().requires_grad_(True)
    tmpl64 = torch.randn(B, V, 3, generator=g, dtype=torch.float64).float().double().requires_grad_(True)
    delta64 = (0.01 * torch.randn(B, V, 3, generator=g, dtype=torch.float64)).float().double().requires_grad_(True)
    gout = torch.randn(B, V, 3, generator=g, dtype=torch.float64)
    gRT = torch.randn(B, 4, 4, generator=g, dtype=torch.float64)
    poses, scales, tmpl, delta = (t.detach().float().to(DEV).requires_grad_(True) for t in (poses64, scales64, tmpl64, delta64))

    st = lbs.compute_rigid_transforms(poses[:, :6], poses[:, 6:], scales)
    check_vals("states", st, rig.states(poses64, scales64))
    check_vals("mats", lbs.compute_rigid_transforms_matrix(poses[:, :6], poses[:, 6:], scales), rig.mats(poses64, scales64))
    t_root, R_root = lbs.compute_root_rigid_transform(poses)
    t64, R64 = rig.root(poses64)
    check_vals("t_root", t_root, t64)
    check_vals("R_root", R_root, R64)
    out, out64 = lbs(poses, scales, tmpl), rig.forward(poses64, scales64, tmpl64)
    check_vals("posed vertices", out, out64)
    got = torch.autograd.grad((out * gout.float().to(DEV)).sum(), [poses, scales, tmpl])
    ref = torch.autograd.grad((out64 * gout).sum(), [poses64, scales64, tmpl64])
    for name, a, b in zip(("motion", "scales", "template"), got, ref):
        check_grad(f"d/d{name} of forward", a, b)

    # the subject's pose (one scale row shared by the frames) and the cage operator
    posed = m.pose(poses, tmpl)
    posed64 = rig.forward(poses64, d64(z["lbs_scale"]).expand(B, -1), tmpl64) * d64(z["global_scaling"])
    check_vals("LBSModule.pose", posed, posed64)
    rot180 = torch.diag(torch.tensor([1.0, -1.0, -1.0, 1.0], dtype=torch.float64))[None]
    cm = torch.tensor([[[0.1, -0.2, 0.3]]], dtype=torch.float64)
    geom, RT = goliath_cage(m, poses, delta, rot180=rot180.float().to(DEV), center_mass=cm.float().to(DEV))
    geom64, RT64 = rig.cage(poses64, d64(z["lbs_scale"]), d64(z["template"]), d64(z["global_scaling"]), rot180, cm, delta64)
    check_vals("goliath_cage geom", geom, geom64)
    check_vals("goliath_cage RT", RT, RT64)
    got = torch.autograd.grad((geom * gout.float().to(DEV)).sum() + (RT * gRT.float().to(DEV)).sum(), [poses, delta])
    ref = torch.autograd.grad((geom64 * gout).sum() + (RT64 * gRT).sum(), [poses64, delta64])
    check_grad("d/dmotion of goliath_cage", got[0], ref[0])
    check_grad("d/ddelta of goliath_cage", got[1], ref[1])


def reference_sequence(m, motion, delta, rot180, center_mass):
    """lib/blueman.py:101-168 replayed call for call through the new classes: skinning (pose with the scaled template), the
    root transform, inv, transform, + center_mass."""
    B = motion.shape[0]
    template = m.lbs_template_verts.expand(B, -1, -1).detach()
    if delta is not None:
        template = (template / 100.0 + delta.expand(B, -1, -1)) * 100.0
    m.lbs_fn.global_scale = m.global_scaling.clone()
    geom = m.pose(motion, template)
    t_root, R_root = m.lbs_fn.compute_root_rigid_transform(motion)
    m.lbs_fn.global_scale = torch.ones_like(m.lbs_fn.global_scale)
    RT = torch.eye(4, device=motion.device)[None].repeat(B, 1, 1)
    RT[:, :3, :3] = R_root
    RT[:, :3, 3] = t_root / 1000.0
    RT = torch.linalg.inv(RT @ rot180)
    geom = geom / 1000
    geom = torch.cat([geom, torch.ones([B, geom.shape[1], 1], device=geom.device)], 2)
    geom = torch.einsum("bji,bki->bkj", RT, geom)[:, :, 0:3]
    return geom + center_mass, RT


def test_goliath_cage_equals_the_reference_call_sequence(golden):
    """Every value of (geom, RT) and of the gradients against the sequence Blueman.get runs, at the forward / gradient bars (the
    operator folds the unit changes into the skinning, so the two are not the same float32 expression)."""
    from d3ga_amd.skeleton_model import default_rot180, goliath_cage
    z = golden("skeleton_cases.npz")
    m = golden_module(z).to(DEV)
    B, V = 3, z["rest"].shape[0]
    g = torch.Generator().manual_seed(7)
    cm = torch.tensor([[[0.05, 0.1, -0.2]]], device=DEV)
    gout = torch.randn(B, V, 3, generator=g).to(DEV)
    for with_delta in (True, False):
        motion = (0.7 * torch.randn(B, 10, generator=g)).to(DEV).requires_grad_(True)
        delta = (0.01 * torch.randn(1, V, 3, generator=g)).to(DEV).requires_grad_(True) if with_delta else None
        geom, RT = goliath_cage(m, motion, delta, center_mass=cm)
        geom_r, RT_r = reference_sequence(m, motion, delta, default_rot180(DEV), cm)
        check_vals("geom vs the call sequence", geom, geom_r.detach().cpu().double())
        check_vals("RT vs the call sequence", RT, RT_r.detach().cpu().double())
        leaves = [motion] + ([delta] if with_delta else [])
        got = torch.autograd.grad((geom * gout).sum(), leaves)
        ref = torch.autograd.grad((geom_r * gout).sum(), leaves)
        for a, b in zip(got, ref):
            check_grad("gradient vs the call sequence", a, b.cpu().double())


def test_reassigned_tables_are_honoured_on_the_next_call(golden):
    from d3ga_amd.skeleton_model import goliath_cage
    z = golden("skeleton_cases.npz")
    m = golden_module(z).to(DEV)
    rig = golden_rig(z)
    poses64 = d64(z["poses"])
    motion = torch.tensor(z["poses"], device=DEV)
    first = m.pose(motion)
    geom_first, _ = goliath_cage(m, motion)
    rng = np.random.default_rng(11)
    V2 = 77                                                     # the cage has its own vertices and tables
    idx = rng.integers(0, 24, size=(V2, 8))
    w = rng.random((V2, 8)).astype(np.float32)
    w /= w.sum(1, keepdims=True)
    tmpl = rng.normal(size=(V2, 3)).astype(np.float32)
    m.lbs_fn.skin_weights = torch.tensor(w, device=DEV)
    m.lbs_fn.skin_indices = torch.tensor(idx, device=DEV)
    m.lbs_template_verts = torch.tensor(tmpl, device=DEV)
    rig.skin_idx, rig.skin_w = torch.tensor(idx), d64(w)
    ref = rig.forward(poses64, d64(z["lbs_scale"]).expand(2, -1), d64(tmpl)[None]) * d64(z["global_scaling"])
    second = m.pose(motion)
    assert tuple(second.shape) == (2, V2, 3) and tuple(first.shape) == (2, 200, 3)
    check_vals("pose after reassignment", second, ref)
    eye = torch.eye(4, dtype=torch.float64)[None]
    geom, _ = goliath_cage(m, motion, rot180=eye.float().to(DEV))
    geom64, _ = rig.cage(poses64, d64(z["lbs_scale"]), d64(tmpl), d64(z["global_scaling"]), eye, torch.zeros(1, 1, 3, dtype=torch.float64))
    check_vals("goliath_cage after reassignment", geom, geom64)
    # an in-place edit of the template is seen as well (the cached template / 100 is keyed by version)
    m.lbs_template_verts.mul_(2.0)
    geom2, _ = goliath_cage(m, motion, rot180=eye.float().to(DEV))
    geom64, _ = rig.cage(poses64, d64(z["lbs_scale"]), 2 * d64(tmpl), d64(z["global_scaling"]), eye, torch.zeros(1, 1, 3, dtype=torch.float64))
    check_vals("goliath_cage after an in-place edit", geom2, geom64)


def test_two_backward_calls_are_bitwise_equal(golden):
    from d3ga_amd.skeleton_model import goliath_cage
    z = golden("skeleton_cases.npz")
    m = golden_module(z).to(DEV)
    g = torch.Generator().manual_seed(3)
    B, V = 4, 200
    motion0 = (0.8 * torch.randn(B, 10, generator=g)).to(DEV)
    delta0 = (0.01 * torch.randn(V, 3, generator=g)).to(DEV)
    gout, gRT = torch.randn(B, V, 3, generator=g).to(DEV), torch.randn(B, 4, 4, generator=g).to(DEV)
    runs = []
    for _ in range(2):
        motion, delta = motion0.clone().requires_grad_(True), delta0.clone().requires_grad_(True)
        geom, RT = goliath_cage(m, motion, delta)
        runs.append(torch.autograd.grad((geom * gout).sum() + (RT * gRT).sum(), [motion, delta]) + (geom.detach(), RT.detach()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert float(runs[0][0].abs().max()) > 0


def test_captured_graph_follows_motion(golden):
    from d3ga_amd.skeleton_model import goliath_cage
    z = golden("skeleton_cases.npz")
    m = golden_module(z).to(DEV)
    g = torch.Generator().manual_seed(5)
    B, V = 2, 200
    motion = (0.5 * torch.randn(B, 10, generator=g)).to(DEV).requires_grad_(True)
    delta = (0.01 * torch.randn(V, 3, generator=g)).to(DEV).requires_grad_(True)
    gout = torch.randn(B, V, 3, generator=g).to(DEV)

    def step():
        geom, RT = goliath_cage(m, motion, delta)
        gm, gd = torch.autograd.grad((geom * gout).sum(), [motion, delta])
        return geom, RT, gm, gd

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):                                 # warm-up: plans, caches and the allocator's pools
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for k in range(2):
        new = (0.5 * torch.randn(B, 10, generator=g)).to(DEV)
        with torch.no_grad():
            motion.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.clone() for t in outs]
        eager = step()
        for name, a, b in zip(("geom", "RT", "d/dmotion", "d/ddelta"), replayed, eager):
            assert torch.equal(a, b), (k, name, float((a - b).abs().max()))


def run_fuzz_case(case):
    from d3ga_amd.skeleton_model import _SkeletonFn, _bind_rows, skeleton_plan
    r = case["rig"]
    f32 = lambda t: t.float().to(DEV).contiguous()
    joint_parents = torch.tensor(r.parents.reshape(-1, 1)).to(DEV)
    plan = skeleton_plan(joint_parents, f32(r.joint_offset), f32(r.joint_rotation), f32(r.transform), f32(r.offsets))
    # the bind state of the float64 rig rounded to float32 is what both sides are handed
    bind = _bind_rows(f32(r.bind), case["J"])
    poses = torch.tensor(case["poses"], device=DEV, requires_grad=True)
    has_scales = case["scales"].shape[1] > 0 and case["seed"] % 5 != 4          # optional input left out in every fifth case
    scales = torch.tensor(case["scales"], device=DEV, requires_grad=True) if has_scales else None
    states, mats, root = _SkeletonFn.apply(plan, bind, poses, scales, None, 2, True, True, 1.0)
    loss = 0
    if case["use_states"]:
        loss = loss + (states[0] * torch.tensor(case["g_states"], device=DEV)).sum()
    if case["use_mats"]:
        loss = loss + (mats[0, :, :, :3, :] * torch.tensor(case["g_mats"], device=DEV)).sum()
    if case["use_root"]:
        loss = loss + (root[1] * torch.tensor(case["g_root"], device=DEV)).sum()
    grads = torch.autograd.grad(loss, [poses] + ([scales] if has_scales else []))
    ref_case = dict(case)
    if not has_scales:
        ref_case["scales"] = np.zeros_like(case["scales"])
    ref = gr.fuzz_eval(ref_case, torch.float64)
    tag = f"seed {case['seed']} J {case['J']} {case['kind']} B {case['B']}"
    states, mats, root = states.detach(), mats.detach(), root.detach()
    errs = dict(states=fwd_err(states[0].cpu().numpy(), ref["states"]), mats=fwd_err(mats[0, :, :, :3, :].cpu().numpy(), ref["mats"]),
                root=fwd_err(root[1].cpu().numpy(), ref["root"]))
    exc = dict(g_poses=elementwise_excess(grads[0].cpu().numpy(), ref["g_poses"]))
    if has_scales:
        exc["g_scales"] = elementwise_excess(grads[1].cpu().numpy(), ref["g_scales"])
    assert not torch.isnan(states).any() and not torch.isnan(mats).any() and not torch.isnan(root).any(), tag
    assert max(errs.values()) <= FWD_BAR, (tag, errs)
    assert max(exc.values()) <= 1.0, (tag, exc)
    return max(errs.values()) / FWD_BAR, max(exc.values())


def run_free_function_case(seed):
    """`solve_skeleton_state` (the kernels' direct mode) and `states_to_matrix` (the per-(frame, joint) kernels) on a fuzz rig."""
    from d3ga_amd import skeleton_model as sm
    case = gr.free_case(seed)
    r, J, B = case["rig"], case["J"], case["B"]
    ref = gr.free_eval(case, torch.float64)
    f32 = lambda t: torch.as_tensor(t).float().to(DEV).contiguous()
    off, rot, par = f32(r.joint_offset), f32(r.joint_rotation), torch.tensor(r.parents.reshape(-1, 1)).to(DEV)
    param = f32(case["param"]).requires_grad_(True)
    states = sm.solve_skeleton_state(param, off, rot, par)
    mats = sm.states_to_matrix(f32(r.bind), states)
    loss = (mats * f32(case["g_mats"])).sum() + ((states * f32(case["g_states"])).sum() if case["use_states"] else 0)
    (got,) = torch.autograd.grad(loss, [param])
    tag = f"free functions: seed {seed} J {J} {case['kind']} B {B} ({B * J} threads)"
    errs = (fwd_err(states.detach().cpu().numpy(), ref["states"]), fwd_err(mats.detach().cpu().numpy(), ref["mats"]))
    exc = elementwise_excess(got.cpu().numpy(), ref["g_param"])
    assert tuple(states.shape) == (B, J, 8) and tuple(mats.shape) == (B, J, 3, 4), tag
    assert max(errs) <= FWD_BAR and exc <= 1.0, (tag, errs, exc)
    return max(errs) / FWD_BAR, exc


def test_fuzz_the_free_functions_against_the_oracle():
    n = int(os.environ.get("D3GA_SKEL_FUZZ_N", "40"))
    first = int(os.environ.get("D3GA_SKEL_FUZZ_FIRST", "1000"))
    worst = (0.0, 0.0)
    for seed in range(first, first + n):
        f, g = run_free_function_case(seed)
        worst = (max(worst[0], f), max(worst[1], g))
    print(f"[skeleton fuzz] free functions, {n} cases from seed {first}: worst forward {worst[0]:.3f} of the bar, worst gradient "
          f"excess {worst[1]:.3f}")


def test_fuzz_against_the_oracle():
    n = int(os.environ.get("D3GA_SKEL_FUZZ_N", "40"))
    first = int(os.environ.get("D3GA_SKEL_FUZZ_FIRST", "1000"))
    worst = (0.0, 0.0)
    for seed in range(first, first + n):
        f, g = run_fuzz_case(gr.fuzz_case(seed))
        worst = (max(worst[0], f), max(worst[1], g))
    print(f"[skeleton fuzz] {n} cases from seed {first}: worst forward {worst[0]:.3f} of the bar, worst gradient excess {worst[1]:.3f}")


def test_largest_rig_and_wide_batch():
    """J = 512 (the kernels' limit) as one deep-capped bushy tree, B = 33."""
    rng = np.random.default_rng(77)
    rig = gr.random_rig(rng, 512, 30, 5, kind="bushy", V=8, max_depth=gr.FUZZ_MAX_DEPTH)
    case = dict(seed=77, rig=rig, J=512, kind="bushy", B=33, poses=rng.uniform(-1, 1, size=(33, 30)).astype(np.float32),
                scales=rng.uniform(-0.1, 0.1, size=(33, 5)).astype(np.float32), use_states=True, use_mats=True, use_root=True,
                g_states=rng.normal(size=(33, 512, 8)).astype(np.float32), g_mats=rng.normal(size=(33, 512, 3, 4)).astype(np.float32),
                g_root=rng.normal(size=(33, 12)).astype(np.float32))
    run_fuzz_case(case)
