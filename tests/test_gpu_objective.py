"""The training objective on the GPU (d3ga_amd/objective.py, csrc/objective.hip) against tests/objective_ref.py: scale_energy
against the reference's own values and the float64 restatement at every edge of its launch, TrainingObjective forward and every
gradient, the terms, the NaN flag, a captured step, and one end-to-end step of the soak test's model.

Bars: forward scalars relative 1e-5 against the float64 restatement of the same float32 inputs -- the derived
bound is (longest sequential run + tree depth) * 2^-24 over non-negative terms: < 40 * 2^-24 for scale_energy at any size used
here, < 100 * 2^-24 for the assembly at its limits; gradients |a - b| <= 1e-3 |b| + 1e-6 max|b| on every element;
reproducibility: equal bits."""
import os
import sys

import numpy as np
import pytest
import torch

import objective_ref as R
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W = R.WEIGHTS
PASS = 1536 * 256 * 4            # floats of one full pass of scale_energy's first stage (D3GA_SCALE_ENERGY_GRID workgroups)


def rel(a, b):
    a, b = (float(x.detach()) if torch.is_tensor(x) else float(x) for x in (a, b))
    return abs(a - b) / abs(b) if b != 0 else abs(a)


def se_inputs(shape, seed, delta=True):
    """log-scales around exp(-4.5) with a spread, and a small network delta, as in a trained avatar"""
    g = torch.Generator().manual_seed(seed)
    s = (-4.5 + 0.5 * torch.randn(shape, generator=g)).to(DEV)
    d = (0.1 * torch.randn(shape, generator=g)).to(DEV) if delta else None
    return s, d


def check_scale_energy(s, d, activation="exp", grads=(True, True)):
    from d3ga_amd.objective import scale_energy
    s = s.detach().requires_grad_(grads[0])
    d = None if d is None else d.detach().requires_grad_(grads[1])
    e = scale_energy(s, d, activation)
    assert tuple(e.shape) == (1,) and e.dtype == torch.float32
    s64 = s.detach().double().requires_grad_(True)
    d64 = None if d is None else d.detach().double().requires_grad_(True)
    want = R.scale_energy(s64, d64, activation)
    r = rel(e, want)
    print(f"scale_energy {tuple(s.shape)} {activation}: {float(e):.9e} vs {float(want):.9e} rel {r:.2e}")
    assert r <= R.FWD_RTOL
    up = torch.tensor([0.7], device=DEV)
    e.backward(up)
    want.backward(up.double())
    for got, ref, need in ((s, s64, grads[0]), (d, d64, grads[1])):
        if got is None:
            continue
        if not need:
            assert got.grad is None
            continue
        assert got.grad.shape == got.shape and R.grad_close(got.grad, ref.grad)
    return e


@pytest.mark.parametrize("name", ["deform_case0.npz", "deform_case1.npz"])
def test_scale_energy_against_the_reference_fixtures(name):
    z = np.load(os.path.join(GOLDEN, name))
    s, d = torch.from_numpy(z["scaling_param"]).to(DEV), torch.from_numpy(z["d_scale"]).to(DEV)
    e = check_scale_energy(s, d)
    assert rel(e, z["scale_energy"][0]) <= R.FWD_RTOL
    z64 = torch.from_numpy(z["grad_scaling_param"])            # (the fixture's gradient includes the deform's: not compared)
    assert z64.shape == s.shape


@pytest.mark.parametrize("P", [1, 2, 5, 257, 1000, PASS // 3 - 1, PASS // 3, PASS // 3 + 1, 500_000])
def test_scale_energy_edge_sizes(P):
    """3P below a 16-byte load, with every tail length, more than one workgroup, around one full pass of the grid, the C3 size"""
    check_scale_energy(*se_inputs((P, 3), P))


@pytest.mark.parametrize("n", [PASS - 1, PASS, PASS + 1])
def test_scale_energy_one_element_around_a_full_pass(n):
    """3P moves in threes; rows of one element put the flat length exactly one below, at and one above a full pass"""
    check_scale_energy(*se_inputs((n, 1), n))


def test_scale_energy_forms():
    from d3ga_amd.objective import scale_energy
    s, d = se_inputs((1000, 3), 7)
    check_scale_energy(s, None)                                 # delta_scale=None
    check_scale_energy(s, d, "none")
    check_scale_energy(s, None, "none")
    check_scale_energy(s, d, grads=(True, False))               # gradient to only one of the two
    check_scale_energy(s, d, grads=(False, True))
    # a view with a storage offset of one float (not 16-byte aligned) and a non-contiguous scaling
    big = torch.zeros(3001, device=DEV)
    big[1:] = s.reshape(-1)
    v = big[1:].view(1000, 3)
    assert v.data_ptr() % 16 == 4
    assert torch.equal(check_scale_energy(v, d), check_scale_energy(s, d))
    wide = torch.zeros(1000, 6, device=DEV)
    wide[:, ::2] = s
    nc = wide[:, ::2]
    assert not nc.is_contiguous()
    assert torch.equal(check_scale_energy(nc, d), check_scale_energy(s, d))
    leaf = wide.clone().requires_grad_(True)                    # the gradient finds its way back through the view
    scale_energy(leaf[:, ::2], d).backward()
    ref = s.clone().requires_grad_(True)
    scale_energy(ref, d).backward()
    assert torch.equal(leaf.grad[:, ::2], ref.grad) and not leaf.grad[:, 1::2].any()
    # logits of -60: the square underflows to 0, the gradient is 0, not NaN
    low = torch.full((5, 3), -60.0, device=DEV, requires_grad=True)
    e = scale_energy(low)
    e.backward()
    assert float(e) == 0.0 and not low.grad.any() and torch.isfinite(low.grad).all()


def test_scale_energy_is_reproducible_and_capturable():
    """Nothing of an eager call's autograd graph may be alive across a capture (d3ga_amd/graph.py): the eager results are kept
    as detached copies, and the captured call gets a leaf of its own."""
    from d3ga_amd.graph import _CAPTURE_MODE
    from d3ga_amd.objective import scale_energy
    s0, d = se_inputs((135_000, 3), 3)

    def run(leaf):
        e = scale_energy(leaf, d)
        e.backward()
        return e.detach().clone(), leaf.grad.clone()
    a, ga = run(s0.clone().requires_grad_(True))
    b, gb = run(s0.clone().requires_grad_(True))
    assert torch.equal(a, b) and torch.equal(ga, gb)
    s = s0.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        scale_energy(s, d).backward()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    s.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode=_CAPTURE_MODE):
        c = scale_energy(s, d)
        c.backward()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(c.detach(), a) and torch.equal(s.grad, ga)


# ---- the assembly ------------------------------------------------------------------------------------------------------------
def check_objective(frames, weights=W):
    from d3ga_amd.objective import TrainingObjective
    obj = TrainingObjective(**weights)
    total = obj(frames)
    assert total.dim() == 0 and total.dtype == torch.float32 and tuple(obj.terms.shape) == (9,) and not obj.terms.requires_grad
    want_total, want = R.objective(frames, weights)
    terms = obj.terms.tolist()
    for i, k in enumerate(R.KEY_ORDER):
        w = float(want[k].detach())
        assert rel(terms[i], w) <= R.FWD_RTOL, (k, terms[i], w)
    assert float(total) == terms[8] and rel(total, want_total.detach()) <= R.FWD_RTOL
    rep = obj.report()
    assert list(rep) == list(R.KEY_ORDER) and list(rep.values()) == terms and all(isinstance(v, float) for v in rep.values())
    lv = R.leaves(frames)
    if lv:
        for _, _, t in lv:
            t.grad = None
        total.backward()
        got = [t.grad.clone() for _, _, t in lv]
        for _, _, t in lv:
            t.grad = None
        want_total.backward()
        for (f, k, t), g in zip(lv, got):
            assert g.shape == t.shape and R.grad_close(g, t.grad), (f, k)
    return obj, total


@pytest.mark.parametrize("B", [1, 2, 4])
@pytest.mark.parametrize("n_cages", [1, 3])
@pytest.mark.parametrize("D", [1, 32, 300])
def test_objective_against_the_oracle(B, n_cages, D):
    check_objective(R.make_frames(B, n_cages, D, seed=1, device=DEV, requires_grad=True))


@pytest.mark.parametrize("kw", [dict(poses=0), dict(fm=False), dict(blur=False), dict(vgg=False),
                                dict(poses=0, fm=False, blur=False, vgg=False), dict(poses=165)])
def test_objective_optional_entries(kw):
    obj, _ = check_objective(R.make_frames(2, 3, 32, seed=2, device=DEV, requires_grad=True, **kw))
    terms = obj.terms.tolist()
    for k, i in (("fm", 3), ("blur", 4), ("vgg", 5)):
        assert (terms[i] == 0.0) == (kw.get(k) is False)
    assert terms[6] == 0.0


def test_objective_views_frozen_inputs_and_the_limits():
    from d3ga_amd.objective import TrainingObjective
    check_objective(R.make_frames(2, 3, 32, seed=3, device=DEV, requires_grad=True, as_views=True))      # views of larger tensors
    frames = R.make_frames(2, 3, 32, seed=4, device=DEV, requires_grad=True)
    for fr in frames:                                            # inputs that do not require a gradient get none
        fr["ssim"] = fr["ssim"].detach()
        fr["frame_encoding"] = fr["frame_encoding"].detach()
    check_objective(frames)
    assert all(fr["ssim"].grad is None and fr["frame_encoding"].grad is None for fr in frames)
    nothing = R.make_frames(1, seed=5, device=DEV)
    assert not TrainingObjective(**W)(nothing).requires_grad
    strided = R.make_frames(1, 3, 32, seed=6, device=DEV)        # a non-contiguous entry
    leaf = torch.zeros(32, 2, device=DEV)
    leaf[:, 0] = strided[0]["frame_encoding"]
    leaf.requires_grad_(True)
    strided[0]["frame_encoding"] = leaf[:, 0]
    strided[0]["_leaf_frame_encoding"] = leaf
    check_objective(strided)
    check_objective(R.make_frames(16, 16, 4096, poses=165, seed=7, device=DEV, requires_grad=True))      # the limits of the table
    # known answer on the device: all-zero inputs
    zeros = {"l1": torch.zeros((), device=DEV), "ssim": torch.zeros((), device=DEV), "sil_l1": torch.zeros((), device=DEV),
             "scale_energy": torch.zeros(3, device=DEV), "fm_energy": torch.zeros(3, device=DEV), "frame_encoding": torch.zeros(32, device=DEV),
             "optimizable_poses": None, "blur_weights": None, "vgg": None}
    want = W["lambda_dssim"] * W["rgb_weight"] + 3.0 * W["fme_weight"]
    assert rel(TrainingObjective(**W)([zeros]), want) <= 2e-7


def test_objective_is_reproducible():
    from d3ga_amd.objective import TrainingObjective
    frames = R.make_frames(4, 3, 300, seed=8, device=DEV, requires_grad=True)
    obj = TrainingObjective(**W)
    outs = []
    for _ in range(2):
        for _, _, t in R.leaves(frames):
            t.grad = None
        total = obj(frames)
        total.backward()
        outs.append((total.clone(), obj.terms.clone(), [t.grad.clone() for _, _, t in R.leaves(frames)]))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert all(torch.equal(a, b) for a, b in zip(outs[0][2], outs[1][2]))
    assert obj.status() == {"nan_seen": False, "first_bad_step": None, "steps": 2}


def test_nan_flag():
    """Plain arithmetic on NaN values: a NaN in an input VALUE reaches the total, the flag keeps the first such step."""
    import time
    from d3ga_amd.objective import TrainingObjective
    good = R.make_frames(2, 3, 32, seed=9, device=DEV, requires_grad=True)
    obj = TrainingObjective(first_iteration=101, **W)
    obj(good).backward()
    obj.check(), obj.poll()
    inf = [dict(fr) for fr in good]
    inf[1]["l1"] = torch.tensor(float("inf"), device=DEV)
    assert torch.isinf(obj(inf))
    obj.check()                                                  # an infinite total does not raise
    assert obj.status() == {"nan_seen": False, "first_bad_step": None, "steps": 2}
    enc = good[0]["frame_encoding"].detach().clone()
    enc[5] = float("nan")
    bad = [dict(fr) for fr in good]
    bad[0]["frame_encoding"] = enc.requires_grad_(True)
    total = obj(bad)
    total.backward()                                             # no kernel minds: the gradient of the NaN element is NaN, the others are numbers
    assert torch.isnan(total) and torch.isnan(enc.grad[5]) and torch.isfinite(enc.grad[:5]).all()
    bad_terms = obj.terms.tolist()
    assert np.isnan(bad_terms[7]) and np.isnan(bad_terms[8]) and np.isfinite(bad_terms[0])
    assert obj.status() == {"nan_seen": True, "first_bad_step": 2, "steps": 3}
    obj(good)                                                    # later finite steps do not clear the flag ...
    nan_l1 = [dict(fr) for fr in good]
    nan_l1[0]["l1"] = torch.tensor(float("nan"), device=DEV)
    assert torch.isnan(obj(nan_l1))                              # ... and a later NaN does not move it
    assert obj.status() == {"nan_seen": True, "first_bad_step": 2, "steps": 5}
    with pytest.raises(ValueError, match="loss is NaN") as ei:
        obj.check()
    msg = str(ei.value)
    assert "iter=103" in msg and "codes_reg=nan" in msg and "total_loss=nan" in msg and f"color_loss={bad_terms[0]:.5f}" in msg
    assert [p.split("=")[0] for p in msg.split(": ")[-1].split(" ")] == list(R.KEY_ORDER)
    # poll never waits: it starts a copy, and raises on a later call once the copy has arrived
    fresh = TrainingObjective(**W)
    fresh(nan_l1)
    t0 = time.perf_counter()
    fresh.poll()
    assert time.perf_counter() - t0 < 0.5
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="loss is NaN: iter=1:"):
        fresh.poll()
    with pytest.raises(ValueError, match="loss is NaN"):         # sticky
        fresh.poll(), torch.cuda.synchronize(), fresh.poll()
    clean = TrainingObjective(**W)
    clean(good)
    for _ in range(3):
        clean.poll()
        torch.cuda.synchronize()


def test_captured_step_over_slot_fed_inputs():
    """objective(frames) + backward() inside a CapturedStep whose inputs are one static buffer: three replays with different
    inputs equal the eager call on the same values bit for bit (total, terms, every gradient); `steps` counts the replays."""
    from d3ga_amd.graph import CapturedStep
    from d3ga_amd.objective import TrainingObjective
    B, n_cages, D, NP = 2, 3, 32, 87
    sizes = [("l1", 1), ("ssim", 1), ("sil_l1", 1), ("scale_energy", n_cages), ("fm_energy", n_cages), ("frame_encoding", D),
             ("optimizable_poses", NP), ("blur_weights", 3), ("vgg", 1)]
    per = sum(n for _, n in sizes)
    buf = torch.zeros(B * per, device=DEV)

    def pack(frames):
        return torch.cat([fr[k].reshape(-1) for fr in frames for k, _ in sizes])

    def run(obj):
        leaf = buf.detach().requires_grad_(True)
        frames, at = [], 0
        for _ in range(B):
            fr = {}
            for k, n in sizes:
                v = leaf[at:at + n]
                fr[k] = v.reshape(()) if k in ("l1", "ssim", "sil_l1", "vgg") else (v.reshape(1, n) if k in ("optimizable_poses", "blur_weights") else v)
                at += n
            frames.append(fr)
        total = obj(frames)
        total.backward()
        return total.detach(), obj.terms, leaf.grad

    sets = [pack(R.make_frames(B, n_cages, D, NP, seed=20 + i, device=DEV)) for i in range(3)]
    eager_obj = TrainingObjective(**W)
    eager = []
    for v in sets:
        buf.copy_(v)
        t, terms, g = run(eager_obj)
        eager.append((t.clone(), terms.clone(), g.clone()))
    del t, terms, g
    buf.copy_(sets[0])
    cap_obj = TrainingObjective(**W)
    cap = CapturedStep(lambda: run(cap_obj), slots={"inputs": buf}, warmup=2)
    before = cap_obj.status()["steps"]
    assert before == 2                                           # the warm-up calls; capturing runs nothing
    for i, v in enumerate(sets):
        t, terms, g = cap.replay(inputs=v)
        torch.cuda.synchronize()
        assert torch.equal(t, eager[i][0]) and torch.equal(terms, eager[i][1]) and torch.equal(g, eager[i][2]), i
        assert cap_obj.report() == {k: x for k, x in zip(R.KEY_ORDER, eager[i][1].tolist())}
        cap_obj.poll()
    assert cap_obj.status() == {"nan_seen": False, "first_bad_step": None, "steps": before + 3}
    nan = sets[1].clone()
    nan[0] = float("nan")
    cap.replay(inputs=nan)
    assert cap_obj.status() == {"nan_seen": True, "first_bad_step": before + 3, "steps": before + 4}
    with pytest.raises(ValueError, match="loss is NaN"):
        cap_obj.check()


def test_end_to_end_step_of_the_soak_model():
    """The soak test's model (tests/test_gpu_train_soak.py: field networks, LBS, cage deform, two renders, L1 + SSIM + silhouette
    + scale regulariser) at its smallest workload, T0: one eager step through scale_energy + TrainingObjective against the same
    step through the torch lines (the float32 restatement), every parameter gradient under the gradient rule."""
    sys.path.insert(0, ROOT)
    import bench
    from d3ga_amd.cage_deform import cage_deform, lbs_cage
    from d3ga_amd.losses import l1_loss, l1_ssim
    from d3ga_amd.objective import TrainingObjective, scale_energy
    from d3ga_amd.rasterizer import geometry_reuse
    from d3ga_amd.renderer import render
    torch.manual_seed(0)
    fr = bench.Frame("T0", torch.device(DEV), 0)
    fr.train_step(with_fields=True, pair=False, scale_weight=175.0)          # creates the field networks and the silhouette target
    g = torch.Generator().manual_seed(4)
    enc = (0.1 * torch.randn(32, generator=g)).to(DEV).requires_grad_(True)
    poses = (0.5 * torch.randn(1, 87, generator=g)).to(DEV).requires_grad_(True)
    p = fr.params
    params = [p["scaling"], p["rotation"], p["opacity"], p["features"], enc, poses] + fr.field_params

    def step(native):
        for q in params:
            q.grad = None
        delta_node = fr.deform_field(fr.canon, fr.pose)
        d_bary, d_rot, d_scale = fr.canon_field(p["rotation"], p["scaling"], fr.barys0, fr.pose)
        tetpoints = lbs_cage(fr.canon, delta_node, fr.joint_mats, fr.skin_idx, fr.skin_w)
        means, cov6 = cage_deform(tetpoints, fr.tetras, fr.tetra_id, fr.barys0, fr.canon_grad, p["scaling"] + d_scale,
                                  p["rotation"] + d_rot, delta_barys=d_bary, scale_activation="exp")
        pkg = {"means3D": means, "cov3D_precomp": cov6, "opacity_logits": p["opacity"], "shs": p["features"], "rgb": None,
               "sh_degree": fr.sh_degree}
        with geometry_reuse():
            img = render(fr.batch, pkg, fr.bg)["render"]
            sil = render(fr.batch, pkg, fr.bg0, colors_precomp=fr.sil_rgb)["render"]
        l1, ssim = l1_ssim(img, fr.target)
        frame = {"l1": l1, "ssim": ssim, "sil_l1": l1_loss(sil, fr.sil_target), "fm_energy": None, "frame_encoding": enc,
                 "optimizable_poses": poses, "blur_weights": None, "vgg": None}
        if native:
            frame["scale_energy"] = scale_energy(p["scaling"], d_scale)
            total = TrainingObjective(**W)([frame])
        else:
            frame["scale_energy"] = R.scale_energy(p["scaling"], d_scale, dtype=torch.float32)
            total = R.objective([frame], W, torch.float32)[0]
        total.backward()
        return float(total), [None if q.grad is None else q.grad.clone() for q in params]

    t_ref, g_ref = step(False)
    t_got, g_got = step(True)
    assert rel(t_got, t_ref) <= R.FWD_RTOL
    assert sum(b is not None for b in g_ref) >= 8
    for i, (a, b) in enumerate(zip(g_got, g_ref)):
        assert (a is None) == (b is None), i
        if b is None:                                            # (a free parameter the networks replace)
            continue
        d = (a - b).abs()
        bar = 1e-3 * b.abs() + 1e-6 * b.abs().max()
        print(f"param {i} {tuple(b.shape)}: worst |a-b| / bar = {float((d / bar.clamp_min(1e-38)).max()):.3f}")
        assert R.grad_close(a, b), i
