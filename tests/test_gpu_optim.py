"""ClipAdam (d3ga_amd/optim.py, csrc/optim.hip) on the GPU against the float64 oracle of tests/optim_ref.py and against
clip_grad_norm_ + torch.optim.Adam.  Needs a real MI355X.

The bars of the one-step test are derived, not tuned:
  grad_norm   relative 2e-6       pairwise float32 summation of N <= 2^31 squares: log2 N x 2^-24 = 1.9e-6
  exp_avg     4e-6 (|b1 m| + |(1 - b1) g'|)
  exp_avg_sq  8e-6 v'             twice the clip coefficient's error + roundings
  p           2e-6 lr + ulp(p')   the normalised update is at most ~3.2 and carries a handful of float32 roundings
and a trajectory of n steps with gradients that do not depend on p is held to n times the bar of p."""
import copy
import sys

import pytest
import torch

from conftest import ROOT
from optim_ref import clip_adam_step_ref, gradient_scale, ulp32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
sys.path.insert(0, ROOT)
BETAS, EPS = (0.9, 0.999), 1e-8


def _leaf(n, gen, offset=False):
    """A float32 parameter of n elements; offset: a contiguous view 4 bytes into a larger buffer (not 16-byte aligned)."""
    if offset:
        buf = torch.randn(n + 1, generator=gen, device=DEV)
        p = torch.nn.Parameter(buf[1:])
        assert p.data_ptr() % 16 == 4 and p.is_contiguous()
        return p
    return torch.nn.Parameter(torch.randn(n, generator=gen, device=DEV))


def _hand_over(opt, params, steps, gen, scales):
    """Install a given Adam state (torch's layout) and return it: exp_avg_sq >= exp_avg^2, as any state Adam has produced."""
    M, V = [], []
    for p, t, s in zip(params, steps, scales):
        if t == 0:
            m, v = torch.zeros_like(p), torch.zeros_like(p)
        else:
            m = s * torch.randn(p.shape, generator=gen, device=DEV)
            v = m * m * (1.0 + torch.rand(p.shape, generator=gen, device=DEV))
        opt.state[p] = {"step": torch.tensor(float(t), dtype=torch.float32, device=DEV), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
        M.append(m); V.append(v)
    return M, V


def _check_one_step(tag, got, want, before, lrs, coef):
    """got / want: (P, M, V) after the step (float32 / float64); before: (M0, G) -- every element is held."""
    (P, M, V), (Pr, Mr, Vr), (M0, G) = got, want, before
    for i in range(len(P)):
        g1 = coef * G[i].double()
        bar_m = 4e-6 * ((BETAS[0] * M0[i].double()).abs() + ((1.0 - BETAS[0]) * g1).abs())
        em, ev, ep = (M[i].double() - Mr[i]).abs(), (V[i].double() - Vr[i]).abs(), (P[i].double() - Pr[i]).abs()
        bar_p = 2e-6 * lrs[i] + ulp32(Pr[i])
        ok = (em <= bar_m).all() & (ev <= 8e-6 * Vr[i]).all() & (ep <= bar_p).all()
        if not bool(ok):
            raise AssertionError(f"{tag} tensor {i} ({P[i].numel()} elements): exp_avg x{float((em / bar_m.clamp_min(1e-300)).max()):.3f}, "
                                 f"exp_avg_sq x{float((ev / (8e-6 * Vr[i]).clamp_min(1e-300)).max()):.3f}, p x{float((ep / bar_p).max()):.3f} of the bar")


def test_one_step_from_a_handed_over_state_against_the_float64_oracle():
    from d3ga_amd.optim import ClipAdam
    special = [1, 3, 5, 4 * 1024 + 1]
    worst = 0.0
    for seed in range(200):
        gen = torch.Generator(device=DEV).manual_seed(1000 + seed)
        cpu = torch.Generator().manual_seed(seed)
        ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=cpu))
        T = ri(1, 40)
        sizes = [special[ri(0, 3)] if ri(0, 4) == 0 else max(1, int(300_000 ** (ri(0, 1000) / 1000.0))) for _ in range(T)]
        if seed % 8 == 0:
            sizes[0] = 300_000
        offset = [ri(0, 5) == 0 for _ in range(T)]
        offset[-1] = offset[-1] or seed % 2 == 0                   # every other seed at least one misaligned view
        n_groups = ri(1, min(T, 5))
        group_of = [ri(0, n_groups - 1) if i >= n_groups else i for i in range(T)]
        group_lr = [10.0 ** -ri(2, 5) * (1 + ri(0, 8)) for _ in range(n_groups)]
        steps = [(0, 1, 10, 100_000)[ri(0, 3)] for _ in range(T)]
        params = [_leaf(n, gen, o) for n, o in zip(sizes, offset)]
        scales = [gradient_scale(seed, i) for i in range(T)]
        G = [s * torch.randn(p.shape, generator=gen, device=DEV) for p, s in zip(params, scales)]
        opt = ClipAdam([{"params": [p for p, k in zip(params, group_of) if k == j], "lr": group_lr[j]} for j in range(n_groups)],
                       betas=BETAS, eps=EPS, max_norm=2.5)
        M0, V0 = _hand_over(opt, params, steps, gen, [gradient_scale(seed + 1, i) for i in range(T)])
        P0 = [p.detach().clone() for p in params]
        for p, g in zip(params, G):
            p.grad = g.clone()
        opt.step()
        lrs = [group_lr[k] for k in group_of]
        Pr, Mr, Vr, Sr, norm = clip_adam_step_ref(P0, G, M0, V0, steps, lrs, [BETAS] * T, [EPS] * T, 2.5)
        rel = abs(float(opt.grad_norm) - float(norm)) / float(norm)
        worst = max(worst, rel)
        assert rel <= 2e-6, (seed, float(opt.grad_norm), float(norm))
        coef = min(1.0, 2.5 / (float(norm) + 1e-6))
        got = ([p.detach() for p in params], [opt.state[p]["exp_avg"] for p in params], [opt.state[p]["exp_avg_sq"] for p in params])
        _check_one_step(f"seed {seed}", got, (Pr, Mr, Vr), (M0, G), lrs, coef)
        assert [int(opt.state[p]["step"]) for p in params] == Sr
        assert all(torch.equal(p.grad, g) for p, g in zip(params, G))            # .grad stays unclipped
    print(f"one step, 200 seeds: worst relative error of grad_norm {worst:.2e}")


def _trajectory_setup(seed=7):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    sizes, offset = [1, 5, 4097, 20_000, 70_001, 3001], [False, False, False, False, False, True]
    group_of, group_lr = [0, 0, 1, 1, 2, 2], [1e-3, 1.6e-4, 5e-3]
    P0 = [_leaf(n, gen, o).detach().clone() for n, o in zip(sizes, offset)]
    grads = [[gradient_scale(it, i) * torch.randn(n, generator=gen, device=DEV) for i, n in enumerate(sizes)] for it in range(100)]
    for it in range(3, 100, 4):
        grads[it][1] = None                                        # torch's skip rule, every fourth step
    return sizes, offset, group_of, group_lr, P0, grads


def _fresh_params(P0, offset):
    out = []
    for p0, o in zip(P0, offset):
        if o:
            buf = torch.zeros(p0.numel() + 1, device=DEV)
            buf[1:] = p0
            out.append(torch.nn.Parameter(buf[1:]))
        else:
            out.append(torch.nn.Parameter(p0.clone()))
    return out


def _groups(params, group_of, group_lr):
    return [{"params": [p for p, k in zip(params, group_of) if k == j], "lr": lr} for j, lr in enumerate(group_lr)]


def _run(kind, params, group_of, group_lr, grads, spacers=True, max_norm=2.5):
    """kind "hip": ClipAdam; "torch": clip_grad_norm_ + torch.optim.Adam.  Gradients are re-created at NEW addresses every step."""
    from d3ga_amd.optim import ClipAdam
    opt = (ClipAdam(_groups(params, group_of, group_lr), betas=BETAS, eps=EPS, max_norm=max_norm) if kind == "hip" else
           torch.optim.Adam(_groups(params, group_of, group_lr), betas=BETAS, eps=EPS, foreach=True))
    keep, moved, last, snaps, norms = [], 0, None, {}, []
    for it, gs in enumerate(grads):
        old = [p.grad for p in params]                             # alive while the new ones are allocated: the addresses must move
        opt.zero_grad(set_to_none=True)
        if spacers:
            keep.append(torch.empty(1000 + 37 * it, device=DEV))   # a spacer, so that the blocks do not simply alternate either
        for p, g in zip(params, gs):
            p.grad = None if g is None else g.clone()
        del old
        now = tuple(p.grad.data_ptr() for p in params if p.grad is not None)
        moved += last is not None and now != last
        last = now
        if kind == "hip":
            opt.step()
            norms.append(opt.grad_norm.clone() if max_norm is not None else None)
        else:
            if max_norm is not None:
                norms.append(torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=True))
            opt.step()
        if it + 1 in (1, 10, 50, 100):
            snaps[it + 1] = [p.detach().clone() for p in params]
    return opt, snaps, norms, moved


def test_trajectory_of_100_steps_against_torch_and_the_oracle():
    sizes, offset, group_of, group_lr, P0, grads = _trajectory_setup()
    lrs = [group_lr[k] for k in group_of]
    T = len(sizes)
    P, M, V, S = [p.double() for p in P0], [torch.zeros_like(p, dtype=torch.float64) for p in P0], [torch.zeros_like(p, dtype=torch.float64) for p in P0], [0] * T
    ref, ref_norms = {}, []
    for it, gs in enumerate(grads):
        P, M, V, S, norm = clip_adam_step_ref(P, gs, M, V, S, lrs, [BETAS] * T, [EPS] * T, 2.5)
        ref_norms.append(float(norm))
        if it + 1 in (1, 10, 50, 100):
            ref[it + 1] = P
    assert S == [100, 75, 100, 100, 100, 100]
    for kind in ("hip", "torch"):
        params = _fresh_params(P0, offset)
        opt, snaps, norms, moved = _run(kind, params, group_of, group_lr, grads)
        assert moved >= 50, moved                                  # the gradients really did move between steps
        for n, Ps in snaps.items():
            for i, (p, r) in enumerate(zip(Ps, ref[n])):
                bar = n * (2e-6 * lrs[i] + ulp32(r))
                err = (p.double() - r).abs()
                assert bool((err <= bar).all()), (kind, n, i, float((err / bar).max()))
        worst = max(abs(float(a) - b) / b for a, b in zip(norms, ref_norms))
        assert worst <= 2e-6, (kind, worst)
        assert [int(opt.state[p]["step"]) for p in params] == S
        print(f"trajectory, {kind}: worst p error {max(float(((p.double() - r).abs() / (100 * (2e-6 * lrs[i] + ulp32(r)))).max()) for i, (p, r) in enumerate(zip(snaps[100], ref[100]))):.3f} of the bar at step 100, norm {worst:.1e}")


def test_two_runs_are_bit_identical():
    sizes, offset, group_of, group_lr, P0, grads = _trajectory_setup(seed=9)
    runs = []
    for _ in range(2):
        params = _fresh_params(P0, offset)
        opt, _, norms, _ = _run("hip", params, group_of, group_lr, grads[:20])
        runs.append(([p.detach().clone() for p in params] + [opt.state[p][k] for p in params for k in ("exp_avg", "exp_avg_sq", "step")], norms))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


def test_state_dict_round_trips_with_torch_adam_and_the_checkpoint_file(tmp_path):
    from d3ga_amd import checkpoint as ck
    from d3ga_amd.optim import ClipAdam
    sizes, offset, group_of, group_lr, P0, grads = _trajectory_setup(seed=13)
    offset = [False] * len(offset)
    lrs = [group_lr[k] for k in group_of]
    make = {"hip": lambda ps: ClipAdam(_groups(ps, group_of, group_lr), betas=BETAS, eps=EPS, max_norm=2.5),
            "torch": lambda ps: torch.optim.Adam(_groups(ps, group_of, group_lr), betas=BETAS, eps=EPS)}

    def steps(kind, opt, params, gs_list):
        for gs in gs_list:
            opt.zero_grad(set_to_none=True)
            for p, g in zip(params, gs):
                p.grad = None if g is None else g.clone()
            if kind == "torch":
                torch.nn.utils.clip_grad_norm_(params, 2.5, foreach=True)
            opt.step()

    for first, second, numeric_step in (("hip", "torch", False), ("torch", "hip", False), ("torch", "hip", True)):
        pa = _fresh_params(P0, offset)
        oa = make[first](pa)
        steps(first, oa, pa, grads[:10])
        sd = copy.deepcopy(oa.state_dict())                        # (as a file would: load_state_dict keeps tensors it need not cast)
        if numeric_step:                                           # older checkpoints hold plain numbers
            for st in sd["state"].values():
                st["step"] = float(st["step"])
        pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
        ob = make[second](pb)
        ob.load_state_dict(sd)
        assert [float(ob.state[p]["step"]) for p in pb] == [float(oa.state[p]["step"]) for p in pa]
        if second == "hip":
            assert all(ob.state[p]["step"].is_cuda and ob.state[p]["step"].dtype == torch.float32 and ob.state[p]["step"].dim() == 0 for p in pb)
        assert set(ob.state[pb[0]]) == {"step", "exp_avg", "exp_avg_sq"}
        steps(first, oa, pa, grads[10:20])
        steps(second, ob, pb, grads[10:20])
        for i, (a, b) in enumerate(zip(pa, pb)):
            bar = 10 * (2e-6 * lrs[i] + ulp32(a.detach()))
            assert bool(((a.double() - b.double()).abs() <= bar).all()), (first, second, i)
        assert [float(ob.state[p]["step"]) for p in pb] == [float(oa.state[p]["step"]) for p in pa]

    # the reference's checkpoint file (models/trainer.py:194-209) with ClipAdam as the optimizer
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.ReLU(), torch.nn.Linear(32, 3)).to(DEV)
    opt = ClipAdam(net.parameters(), lr=1e-3, max_norm=2.5)
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[2, 4], gamma=0.33)
    x = torch.randn(64, 16, device=DEV)
    for _ in range(3):
        opt.zero_grad()
        net(x).square().mean().backward()
        opt.step(); sch.step()
    ck.save_checkpoint(str(tmp_path), 3, net, opt, sch)
    net2 = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.ReLU(), torch.nn.Linear(32, 3)).to(DEV)
    opt2 = ClipAdam(net2.parameters(), lr=1e-3, max_norm=2.5)
    sch2 = torch.optim.lr_scheduler.MultiStepLR(opt2, milestones=[2, 4], gamma=0.33)
    assert ck.load_checkpoint(str(tmp_path), net2, opt2, sch2) == 3
    assert opt2.param_groups[0]["lr"] == pytest.approx(0.33e-3)
    for a, b in zip(net.parameters(), net2.parameters()):
        assert torch.equal(opt.state[a]["exp_avg"], opt2.state[b]["exp_avg"]) and float(opt2.state[b]["step"]) == 3.0
    for n_, o_, s_ in ((net, opt, sch), (net2, opt2, sch2)):
        for _ in range(2):
            o_.zero_grad()
            n_(x).square().mean().backward()
            o_.step(); s_.step()
    assert all(torch.allclose(a, b, rtol=1e-5, atol=1e-7) for a, b in zip(net.parameters(), net2.parameters()))


def test_captured_step_follows_the_scheduler_and_equals_eager():
    from d3ga_amd import rasterizer as R
    from d3ga_amd.graph import CapturedStep
    from d3ga_amd.losses import l1_loss
    from d3ga_amd.optim import ClipAdam
    from d3ga_amd.renderer import render
    from util import scene_inputs
    inp = scene_inputs("T1", scale_mult=3.0)
    bg = torch.ones(3, device=DEV)
    fixed = {"cov3D_precomp": inp["cov6"].to(DEV), "opacities": inp["opacities"].to(DEV), "shs": None, "sh_degree": 0}
    with torch.no_grad():
        target = render(inp["batch"], dict(fixed, means3D=inp["means3D"].to(DEV), rgb=(0.7 * inp["rgb"]).to(DEV)), bg)["render"].clone()
    d = R.last_counters()["D"]

    def make(real):
        means = inp["means3D"].to(DEV).clone().requires_grad_(True)
        rgb = inp["rgb"].to(DEV).clone().requires_grad_(True)
        params = [means, rgb]
        opt = ClipAdam([{"params": [means], "lr": 1e-4}, {"params": [rgb], "lr": 1e-2}], max_norm=2.5)
        sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[5, 9], gamma=0.33)
        gen = torch.Generator(device=DEV).manual_seed(5)
        given = [30.0 * torch.randn(p.shape, generator=gen, device=DEV) for p in params]

        def step_fn():
            if real:
                means.grad = rgb.grad = None
                loss = l1_loss(render(inp["batch"], dict(fixed, means3D=means, rgb=rgb), bg)["render"], target)
                loss.backward()
            else:
                means.grad, rgb.grad = given
            opt.step()
        return params, opt, sched, step_fn

    R.set_capacity_policy("static", 2 * d)
    try:
        for real in (True, False):
            params, opt, sched, step_fn = make(real)
            cap = CapturedStep(step_fn, params=params, warmup=2)             # two eager steps, then the capture (which runs nothing)
            for _ in range(12):
                cap.replay()
                sched.step()
                opt.flush_hyperparams()
            twin, topt, tsched, tstep = make(real)
            for _ in range(2):
                tstep()
            for _ in range(12):
                tstep()
                tsched.step()
            torch.cuda.synchronize()
            assert opt.param_groups[1]["lr"] == pytest.approx(1e-2 * 0.33 * 0.33) and topt.param_groups[1]["lr"] == opt.param_groups[1]["lr"]
            assert [float(opt.state[p]["step"]) for p in params] == [14.0, 14.0] == [float(topt.state[p]["step"]) for p in twin]
            for a, b in zip(params, twin):
                if real:     # float atomics in the compositing backward: the rasterizer's own run-to-run bar (test_gpu_train_soak.py)
                    assert float((a - b).abs().max() / b.abs().max()) < 2e-3
                else:
                    assert torch.equal(a, b)
            assert float((params[1] - inp["rgb"].to(DEV)).abs().max()) > 1e-3               # the replays did train
            if not real:
                assert torch.equal(opt.grad_norm, topt.grad_norm)
                for p, q in zip(params, twin):
                    assert torch.equal(opt.state[p]["exp_avg_sq"], topt.state[q]["exp_avg_sq"])
    finally:
        R.set_capacity_policy("auto")


def test_without_clipping_it_is_plain_adam():
    from d3ga_amd.optim import ClipAdam
    for seed in range(5):
        gen = torch.Generator(device=DEV).manual_seed(50 + seed)
        sizes, offset = [1, 3, 5, 4097, 50_000, 1234], [False, False, False, False, False, True]
        group_of, group_lr = [0, 1, 1, 2, 0, 2], [1e-3, 4e-5, 7e-3]
        lrs = [group_lr[k] for k in group_of]
        steps = [0, 1, 10, 100_000, 10, 1]
        P0 = [_leaf(n, gen, o).detach().clone() for n, o in zip(sizes, offset)]
        G = [gradient_scale(seed, i) * torch.randn(n, generator=gen, device=DEV) for i, n in enumerate(sizes)]
        res = {}
        for kind in ("none", "huge", "torch"):
            params = _fresh_params(P0, offset)
            groups = _groups(params, group_of, group_lr)
            opt = torch.optim.Adam(groups, betas=BETAS, eps=EPS) if kind == "torch" else \
                ClipAdam(groups, betas=BETAS, eps=EPS, max_norm=None if kind == "none" else 1e30)
            M0, V0 = _hand_over(opt, params, steps, torch.Generator(device=DEV).manual_seed(90 + seed), [gradient_scale(seed + 1, i) for i in range(6)])
            if kind == "torch":
                for p in params:
                    opt.state[p]["step"] = opt.state[p]["step"].cpu()             # (torch keeps it on the host unless capturable)
            for p, g in zip(params, G):
                p.grad = g.clone()
            opt.step()
            res[kind] = ([p.detach() for p in params], [opt.state[p]["exp_avg"] for p in params], [opt.state[p]["exp_avg_sq"] for p in params])
            if kind == "none":
                assert opt.grad_norm is None or float(opt.grad_norm) == 0.0       # nothing computed, nothing reported
        for a, b in zip(res["none"], res["huge"]):
            assert all(torch.equal(x, y) for x, y in zip(a, b))                   # a coefficient of exactly 1
        want = tuple([t.double() for t in part] for part in res["torch"])
        _check_one_step(f"seed {seed} vs torch", res["none"], want, (M0, G), lrs, 1.0)
        Pr, Mr, Vr, _, norm = clip_adam_step_ref(P0, G, M0, V0, steps, lrs, [BETAS] * 6, [EPS] * 6, None)
        assert norm is None
        _check_one_step(f"seed {seed} vs oracle", res["none"], (Pr, Mr, Vr), (M0, G), lrs, 1.0)


def test_sparse_and_non_contiguous_gradients():
    from d3ga_amd.optim import ClipAdam
    emb = torch.nn.Embedding(10, 4, sparse=True).to(DEV)
    opt = ClipAdam(emb.parameters(), max_norm=2.5)
    emb(torch.tensor([1, 2], device=DEV)).sum().backward()
    with pytest.raises(ValueError, match="sparse"):
        opt.step()
    p = torch.nn.Parameter(torch.zeros(4, 6, device=DEV))
    q = torch.nn.Parameter(torch.zeros(4, 6, device=DEV))
    g = torch.randn(6, 4, device=DEV).t()
    assert not g.is_contiguous()
    p.grad, q.grad = g, g.contiguous()
    ClipAdam([p], max_norm=2.5).step()                          # made contiguous in eager mode
    ClipAdam([q], max_norm=2.5).step()
    assert torch.equal(p, q) and float(p.abs().max()) > 0


def test_c4_hundred_training_steps_with_clip_adam():
    """The soak of tests/test_gpu_train_soak.py with ClipAdam in place of clip_grad_norm_ + torch.optim.Adam."""
    import bench
    from d3ga_amd import rasterizer as R
    from d3ga_amd.optim import ClipAdam
    from test_gpu_train_soak import _reachable_targets
    torch.manual_seed(0)
    frame = bench.Frame("C4", torch.device(DEV), 0)
    _reachable_targets(frame)
    step = lambda: frame.train_step(with_fields=True, pair=False, scale_weight=175.0)
    step()
    params = [q for q in list(frame.params.values()) + frame.field_params if q.grad is not None]
    opt = ClipAdam(params, lr=1e-3, max_norm=2.5)
    losses = []
    for it in range(100):
        opt.zero_grad(set_to_none=True)
        loss = step()
        opt.step()
        if it % 10 == 0 or it == 99:
            cnt = R.last_counters()
            assert not cnt["overflow"], cnt
            assert torch.isfinite(loss) and torch.isfinite(opt.grad_norm), (it, float(loss), float(opt.grad_norm))
            assert all(torch.isfinite(q).all() for q in params), it
            losses.append(float(loss.detach()))
    print("C4 soak with ClipAdam: loss", [round(v, 5) for v in losses], "last grad_norm", float(opt.grad_norm))
    assert losses[-1] <= 0.8 * losses[0], losses


def test_a_table_longer_than_the_grid_against_the_oracle():
    """More chunks than the launch has workgroups (2048): every workgroup walks the table more than once, which no other
    checked case does (the C3 parameter set is of this kind)."""
    from d3ga_amd.optim import ClipAdam, n_chunks_of
    gen = torch.Generator(device=DEV).manual_seed(77)
    sizes, offset, group_of, group_lr = [17_500_003, 4097, 1, 100_001], [False, False, False, True], [0, 1, 1, 0], [1e-3, 3e-4]
    assert n_chunks_of(sizes[0]) > 2048
    lrs = [group_lr[k] for k in group_of]
    for steps in ([0, 0, 0, 0], [10, 100_000, 1, 10]):
        params = [_leaf(n, gen, o) for n, o in zip(sizes, offset)]
        G = [gradient_scale(1 if steps[0] else 0, i) * torch.randn(p.shape, generator=gen, device=DEV) for i, p in enumerate(params)]
        opt = ClipAdam(_groups(params, group_of, group_lr), betas=BETAS, eps=EPS, max_norm=2.5)
        M0, V0 = _hand_over(opt, params, steps, gen, [gradient_scale(3, i) for i in range(4)])
        P0 = [p.detach().clone() for p in params]
        for p, g in zip(params, G):
            p.grad = g.clone()
        opt.step()
        Pr, Mr, Vr, Sr, norm = clip_adam_step_ref(P0, G, M0, V0, steps, lrs, [BETAS] * 4, [EPS] * 4, 2.5)
        assert abs(float(opt.grad_norm) - float(norm)) <= 2e-6 * float(norm)
        got = ([p.detach() for p in params], [opt.state[p]["exp_avg"] for p in params], [opt.state[p]["exp_avg_sq"] for p in params])
        _check_one_step(f"steps {steps}", got, (Pr, Mr, Vr), (M0, G), lrs, min(1.0, 2.5 / (float(norm) + 1e-6)))
        assert [int(opt.state[p]["step"]) for p in params] == Sr
        del opt, params, G, M0, V0, P0, Pr, Mr, Vr, got
        torch.cuda.empty_cache()


def test_gradients_are_released_by_zero_grad_and_a_steady_loop_uploads_nothing():
    """The optimizer keeps no reference to the gradients of the last step: zero_grad() frees them (as with torch.optim.Adam), the
    next backward gets the same blocks, and the tables are neither rebuilt nor uploaded again."""
    from d3ga_amd.optim import ClipAdam
    sizes = [3_000_000, 1_000_003, 70_001, 257]
    params = [torch.nn.Parameter(torch.zeros(n, device=DEV)) for n in sizes]
    grad_bytes = 4 * sum(sizes)
    opt = ClipAdam(params, lr=1e-3, max_norm=2.5)

    def backward():
        for p in params:
            p.grad = torch.full_like(p, 0.01)                      # a fresh allocation per step, as autograd makes
    backward()
    opt.step()
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    opt.zero_grad()                                                # set_to_none=True is torch's default
    assert held - torch.cuda.memory_allocated() >= grad_bytes, (held, torch.cuda.memory_allocated(), grad_bytes)
    for _ in range(3):
        backward(); opt.step(); opt.zero_grad()
    uploads = opt.plan_uploads
    for _ in range(10):
        backward(); opt.step(); opt.zero_grad()
    assert opt.plan_uploads == uploads, (uploads, opt.plan_uploads)
    # ... and with gradients that autograd itself allocates
    torch.manual_seed(1)
    net = torch.nn.Sequential(torch.nn.Linear(64, 256), torch.nn.ReLU(), torch.nn.Linear(256, 256), torch.nn.ReLU(), torch.nn.Linear(256, 3)).to(DEV)
    x = torch.randn(512, 64, device=DEV)
    opt = ClipAdam(net.parameters(), lr=1e-3, max_norm=2.5)
    first = None
    for it in range(13):
        loss = net(x).square().mean()
        loss.backward()
        opt.step()
        opt.zero_grad()
        if it == 2:
            uploads, first = opt.plan_uploads, float(loss)
    assert opt.plan_uploads == uploads, (uploads, opt.plan_uploads)
    assert float(loss) < first


def test_what_a_capture_refuses():
    from d3ga_amd.optim import ClipAdam

    def capture(fn):
        graph = torch.cuda.CUDAGraph()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
            fn()
        return graph

    def fresh(stepped):
        p = torch.nn.Parameter(torch.ones(4, 6, device=DEV))
        opt = ClipAdam([p], lr=1e-3, max_norm=2.5)
        p.grad = torch.full_like(p, 0.5)
        if stepped:
            opt.step()
        torch.cuda.synchronize()
        return p, opt
    p, opt = fresh(stepped=False)
    with pytest.raises(RuntimeError, match="state would be created inside a capture"):
        capture(opt.step)
    p, opt = fresh(stepped=True)
    p.grad = torch.full((6, 4), 0.5, device=DEV).t()
    assert not p.grad.is_contiguous()
    with pytest.raises(ValueError, match="non-contiguous gradient inside a capture"):
        capture(opt.step)
    p, opt = fresh(stepped=True)
    opt.param_groups[0]["lr"] = 5e-4
    with pytest.raises(RuntimeError, match="hyperparameters changed inside a capture"):
        capture(opt.step)
    # two captures back to back: the second finds no pinned table prepared and says so; one flush_hyperparams() later it works
    p, opt = fresh(stepped=True)
    g1 = capture(opt.step)
    with pytest.raises(RuntimeError, match="second capture"):
        capture(opt.step)
    opt.flush_hyperparams()
    g2 = capture(opt.step)
    torch.cuda.synchronize()
    before = p.detach().clone()
    g1.replay(); g2.replay()
    torch.cuda.synchronize()
    assert float(opt.state[p]["step"]) == 3.0 and float((p - before).abs().max()) > 0
