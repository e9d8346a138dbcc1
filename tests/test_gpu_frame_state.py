"""Frame state on the GPU (d3ga_amd/frame_state.py, csrc/frame_state.hip): the lookup against the fixture of the reference's own
Embedding (tests/golden/frame_state_cases.npz) and the float64 restatement (frame_state_ref.py), the mean, the row cache against
a Python model of a write-back cache, the lazy-Adam equivalence with a real nn.ParameterDict, the same step inside a captured
graph that follows a device cell, the pose-gradient chain and the checkpoint round trip."""
import numpy as np
import pytest
import torch
from torch import nn

import frame_state_ref as R
from test_frame_state_host import cases, smplx

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEQ = [0, 3, 3, 1, 0, 4, 3]                                  # frames of the training runs below; row 2 is never selected
NAMES = ("optimizable_rotations", "optimizable_translations", "optimizable_poses")


def f64(t):
    return t.detach().double().cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------------------
# lookup
# ------------------------------------------------------------------------------------------------------------------------------
def test_lookup_against_the_fixture():
    """Untouched rows and looked-up rows at or below max_norm: the table's bits.  Scaled rows and the output: rtol 1e-6 (the
    norm is summed in another order than the CPU's, a few ulp of the scale).  The dense gradient: the fixture's bits where a row
    is hit once or twice (a two-term sum has no order), rtol 1e-6 of float64 where it is hit three times (the N = 1 cases, whose
    upstream gradient has one sign)."""
    from d3ga_amd.frame_state import code_lookup
    for c in cases():
        n, mx = int(c["n"]), float(c["max_norm"])
        w = torch.from_numpy(c["before"]).to(DEV).requires_grad_(True)
        v0 = w._version
        out = code_lookup(w, torch.from_numpy(c["idx"]).to(DEV), mx)
        assert w._version > v0                               # caches keyed by the version see the in-place renorm
        out.backward(torch.from_numpy(c["dout"]).to(DEV))
        torch.cuda.synchronize()
        after, rows = w.detach().cpu().numpy(), R.clamp_rows(c["idx"], n)
        for r in range(n):
            if np.array_equal(c["after"][r], c["before"][r]):
                assert np.array_equal(after[r], c["before"][r]), (n, c["d"], r)
            else:
                assert not np.array_equal(after[r], c["before"][r])
                np.testing.assert_allclose(after[r], c["after"][r], rtol=1e-6, atol=0)
        np.testing.assert_allclose(out.detach().cpu().numpy(), c["out"], rtol=1e-6, atol=0)
        assert np.array_equal(out.detach().cpu().numpy(), after[rows])          # the copies ARE the table's rows, all equal
        hits = np.bincount(rows, minlength=n)
        got = w.grad.cpu().numpy()
        ref = R.code_lookup_bwd(c["dout"], c["idx"], n)
        for r in range(n):
            if hits[r] <= 2:
                assert np.array_equal(got[r], c["dweight"][r]), (n, c["d"], r)
            else:
                np.testing.assert_allclose(got[r], ref[r], rtol=1e-6, atol=0)
            if hits[r] == 0:
                assert not got[r].any()


def test_gradient_of_sixteen_equal_indices_and_zeros_over_nans():
    """B = 16, all equal: a 16-term sum in increasing b against float64, rtol 1e-6 -- the terms share a sign, so the sum's
    condition number is 1 and 15 roundings of 2^-24 stay below the bar.  Every element of dtable is WRITTEN: rows nobody names
    are exact zeros although the buffer held NaNs."""
    from d3ga_amd import _lib
    g = torch.Generator().manual_seed(16)
    for n, d in ((7, 32), (7, 5)):                           # the 16-byte and the scalar kernel
        dout = (torch.rand(16, d, generator=g) + 0.25).to(DEV)
        idx = torch.full((16,), 4, dtype=torch.int32, device=DEV)
        dtable = torch.full((n, d), float("nan"), device=DEV)
        _lib.check(_lib.lib().d3ga_code_lookup_bwd(_lib.dptr(dout), _lib.dptr(idx), n, d, 16, _lib.dptr(dtable), _lib.stream_handle()), "bwd")
        got = dtable.cpu().numpy()
        np.testing.assert_allclose(got[4], f64(dout).sum(0), rtol=1e-6, atol=0)
        assert not np.delete(got, 4, axis=0).any() and np.isfinite(got).all()
        again = torch.full((n, d), float("nan"), device=DEV)
        _lib.check(_lib.lib().d3ga_code_lookup_bwd(_lib.dptr(dout), _lib.dptr(idx), n, d, 16, _lib.dptr(again), _lib.stream_handle()), "bwd")
        assert torch.equal(again, dtable)


def rows_off_the_threshold(n, d, mx, seed):
    """Rows with norms of 0.5 mx and 1.5 mx in turn: the renorm decision hangs on no rounding."""
    t = torch.randn(n, d, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    t = t / t.norm(dim=1, keepdim=True) * (mx * (0.5 + (torch.arange(n) % 2)))[:, None]
    return t.float()


@pytest.mark.parametrize("n,d,idx", [(1031, 3, [1030, 0, 517, 5000, -4]), (3, 4096, [1]), (3, 4096, [2, 1, 2]), (6, 32, [5])])
def test_lookup_edges(n, d, idx):
    """N D no multiple of 4 or of the block (1031 x 3: the scalar gradient kernel over several workgroups), the widest row
    (D = 4096: sixteen elements per thread), B = 1; against the float64 restatement with the fixture's bars."""
    from d3ga_amd.frame_state import code_lookup
    mx = float(d)
    before = rows_off_the_threshold(n, d, mx, 100 + d)
    w = before.to(DEV).requires_grad_(True)
    dout = torch.randn(len(idx), d, generator=torch.Generator().manual_seed(d))
    out = code_lookup(w, idx, mx)
    out.backward(dout.to(DEV))
    ref_after, ref_out = R.code_lookup_fwd(before.numpy(), idx, mx)
    after, rows = w.detach().cpu().numpy(), R.clamp_rows(idx, n)
    scaled = sorted(r for r in set(rows.tolist()) if r % 2 == 1)
    assert scaled
    keep = np.ones(n, bool)
    keep[scaled] = False
    assert np.array_equal(after[keep], before.numpy()[keep])
    np.testing.assert_allclose(after[scaled], ref_after[scaled], rtol=1e-6, atol=0)
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref_out, rtol=1e-6, atol=0)
    got, ref = w.grad.cpu().numpy(), R.code_lookup_bwd(dout.numpy(), idx, n)
    assert np.array_equal(got, ref.astype(np.float32))       # at most two hits per row: the float32 sum is the rounded float64 one
    assert got.shape == (n, d)


def test_lookup_index_forms_max_norm_none_and_second_forward():
    from d3ga_amd.frame_state import Embedding, code_lookup
    before = rows_off_the_threshold(6, 32, 32.0, 1)
    outs, tables = [], []
    for form in (5, [5], torch.tensor([5]), torch.tensor([5], device=DEV), torch.tensor([5], dtype=torch.int32, device=DEV)):
        w = before.to(DEV)
        outs.append(code_lookup(w, form, 32.0))
        tables.append(w)
    assert all(torch.equal(o, outs[0]) for o in outs) and all(torch.equal(t, tables[0]) for t in tables)
    assert not torch.equal(tables[0][5].cpu(), before[5]) and tuple(outs[0].shape) == (1, 32)
    # a cell is read when the kernel runs; an index past either end is clamped
    cell = torch.tensor([0], dtype=torch.int32, device=DEV)
    w = before.to(DEV)
    for i, row in ((4, 4), (-3, 0), (77, 5), (2, 2)):
        cell.fill_(i)
        assert torch.equal(code_lookup(w, cell, None)[0].cpu(), before[row])
    assert torch.equal(w.cpu(), before)                      # max_norm=None: no row is touched, whatever its norm
    # A second forward on a renormed table changes nothing.  Cases where that is a statement about the number formats, not
    # about luck: (6,8,0,0,0) with max_norm 5 has norm 10, 10 + 1e-7 rounds to 10, the scale is exactly 0.5 and the result
    # (3,4,0,0,0) has norm exactly 5, which is not > 5; a one-element row |x| > 1 becomes x fl(1 / (|x| + 1e-7)), which rounds
    # to at most 1 in magnitude (1 + 2^-24 is a tie that goes to 1), and 1 is not > 1.
    for c in (cases()[6], cases()[0], cases()[1]):
        w = torch.from_numpy(c["before"]).to(DEV)
        idx = torch.from_numpy(c["idx"]).to(DEV)
        o1 = code_lookup(w, idx, float(c["max_norm"]))
        t1 = w.clone()
        o2 = code_lookup(w, idx, float(c["max_norm"]))
        assert torch.equal(w, t1) and torch.equal(o1, o2)
    # the module: shape, and the reference's checkpoint key
    emb = Embedding(6, 4, height=2, width=4).to(DEV)
    assert tuple(emb(torch.tensor([1, 1, 3], device=DEV)).shape) == (3, 4, 2, 4)


# ------------------------------------------------------------------------------------------------------------------------------
# average()
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(1, 32), (1025, 5), (1025, 32), (20_000, 32), (37, 300)])
def test_average(n, d):
    """float64 accumulation, one rounding at the end: rtol 1e-6 even where the mean of zero-mean codes cancels"""
    from d3ga_amd.frame_state import Embedding
    torch.manual_seed(n + d)
    a, b = Embedding(n, d).to(DEV), Embedding(n, d).to(DEV)
    with torch.no_grad():
        b.frame_embs.weight.copy_(a.frame_embs.weight)
    got = a.average()
    assert tuple(got.shape) == (1, d) and not got.requires_grad
    np.testing.assert_allclose(got.cpu().numpy(), R.table_mean(f64(a.frame_embs.weight)), rtol=1e-6, atol=0)
    assert torch.equal(got, b.average())                     # two computations: the same bits
    assert a.average() is got                                # an evaluation loop computes it once


def test_average_cache_is_dropped_by_a_weight_update_and_by_a_replay():
    from d3ga_amd.frame_state import Embedding
    from d3ga_amd.graph import CapturedStep
    emb = Embedding(50, 8).to(DEV)
    w = emb.frame_embs.weight
    a0 = emb.average().clone()
    with torch.no_grad():
        w.add_(1.0)                                          # bumps the version counter
    a1 = emb.average().clone()
    np.testing.assert_allclose(a1.cpu().numpy(), a0.cpu().numpy() + 1.0, rtol=1e-6)
    cap = CapturedStep(lambda: w.data.mul_(2.0), warmup=1)   # a replay writes the weight in place and bumps no version
    stale = emb.average()
    cap.replay()
    fresh = emb.average()
    assert fresh is not stale
    np.testing.assert_allclose(fresh.cpu().numpy(), R.table_mean(f64(w)), rtol=1e-6, atol=0)
    assert float((fresh - a1).abs().max()) > 0.5             # (the replay did change the table)


# ------------------------------------------------------------------------------------------------------------------------------
# row cache
# ------------------------------------------------------------------------------------------------------------------------------
def test_row_cache_kernels_against_the_model():
    """Widths {1, 3, 87, 165} in ONE descriptor; the stage is modified between the selects of [2, 2, 0, 6, 2]."""
    from d3ga_amd import _lib
    L, n = _lib.lib(), 7
    g = torch.Generator().manual_seed(9)
    widths = (1, 3, 87, 165)
    tables = [torch.randn(n, w, generator=g).to(DEV) if w > 1 else torch.randn(n, generator=g).to(DEV) for w in widths]
    stages = [torch.zeros(1, w, device=DEV) if w > 1 else torch.zeros((), device=DEV) for w in widths]
    model = R.RowCacheModel([(t.cpu().numpy().copy(), s.cpu().numpy().copy()) for t, s in zip(tables, stages)])
    desc = (_lib.RowPair * 4)(*[_lib.RowPair(t.data_ptr(), s.data_ptr(), w, n) for t, s, w in zip(tables, stages, widths)])
    idx = torch.zeros(1, dtype=torch.int32, device=DEV)
    prev = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)

    def same():
        torch.cuda.synchronize()
        for (mt, ms), t, s in zip(model.pairs, tables, stages):
            assert torch.equal(t.cpu(), torch.from_numpy(mt)) and torch.equal(s.cpu(), torch.from_numpy(ms))
        assert int(prev) == model.prev and int(flag) == model.flag

    def select(i):
        idx.fill_(i)
        _lib.check(L.d3ga_row_cache_select(desc, 4, _lib.dptr(idx), _lib.dptr(prev), _lib.dptr(flag), _lib.stream_handle()), "select")
        model.select(i)
        same()

    def flush():
        _lib.check(L.d3ga_row_cache_flush(desc, 4, _lib.dptr(prev), _lib.dptr(flag), _lib.stream_handle()), "flush")
        model.flush()
        same()

    for k, i in enumerate([2, 2, 0, 6, 2]):
        select(i)                                            # (the second 2: idx == prev, nothing moves, the stage keeps its edits)
        for s, (_, ms) in zip(stages, model.pairs):
            s.add_(k + 1.0)
            ms += k + 1.0
    assert not torch.equal(tables[2][2].cpu(), stages[2][0].cpu())
    flush()
    flush()                                                  # idempotent
    assert torch.equal(tables[2][2], stages[2][0]) and int(flag) == 0
    for bad in (n, -1):                                      # nothing moves, prev stays, the flag is set and stays
        flag.zero_()
        model.flag = 0
        select(bad)
        assert int(flag) == 1 and int(prev) == 2
    select(3)
    assert int(flag) == 1 and int(prev) == 3


def test_row_cache_module():
    from d3ga_amd.frame_state import RowCache
    entries = {f"k{i}": torch.full((1, 4), float(i)) for i in range(5)}
    c = RowCache(entries, "poses_of_a_test").to(DEV)
    c.select("k3")
    assert torch.equal(c.current.detach().cpu(), entries["k3"])
    with torch.no_grad():
        c.current.add_(0.5)
    c.select(torch.tensor([1], dtype=torch.int32, device=DEV))
    assert torch.equal(c.table[3].cpu(), entries["k3"][0] + 0.5) and torch.equal(c.current.detach().cpu(), entries["k1"])
    with torch.no_grad():
        c.current.mul_(3.0)
    sd = c.state_dict()                                      # flushes
    assert torch.equal(sd["k1"].cpu(), 3.0 * entries["k1"]) and list(sd) == list(entries)
    c.check()
    c.select(torch.tensor([5], dtype=torch.int32, device=DEV))
    assert torch.equal(c.current.detach().cpu(), 3.0 * entries["k1"])
    with pytest.raises(IndexError, match="poses_of_a_test"):
        c.check()
    cpu = c.cpu()                                            # a module moved to the host for its checkpoint
    with torch.no_grad():
        cpu.current.add_(1.0)
    assert torch.equal(cpu.state_dict()["k1"], 3.0 * entries["k1"] + 1.0)


# ------------------------------------------------------------------------------------------------------------------------------
# the lazy Adam of a ParameterDict, eager and captured
# ------------------------------------------------------------------------------------------------------------------------------
def quadratic(x, q):
    """a fixed random quadratic of a (1,D) row: element-wise ops and sums only"""
    w, c, v = q
    return (w * (x - c) ** 2).sum() + (v * x[:, :-1] * x[:, 1:]).sum()


def problem():
    g = torch.Generator().manual_seed(21)
    q = {name: tuple(t.to(DEV) for t in (torch.rand(1, d, generator=g) + 0.5, torch.randn(1, d, generator=g), torch.randn(1, d - 1, generator=g)))
         for name, d in zip(NAMES + ("code",), (3, 3, 87, 8))}
    return smplx(5, 87), q


def new_embedding():
    from d3ga_amd.frame_state import Embedding
    torch.manual_seed(4)
    return Embedding(5, 8, std=3.0).to(DEV)                  # std 3: rows on both sides of max_norm = 8


_runs = {}


def run(mode):
    """The frames of SEQ through ClipAdam(max_norm=2.5): mode "dict" -- the reference's nn.ParameterDict, one parameter per
    frame, picked on the host; "eager" -- FramePoses with attach, selected by a host index; "captured" -- the same step
    captured once and replayed with the frame in a device cell.  -> tables, moments and steps per row, the code table."""
    if mode in _runs:
        return _runs[mode]
    from d3ga_amd.frame_state import FramePoses
    from d3ga_amd.graph import CapturedStep
    from d3ga_amd.optim import ClipAdam
    data, q = problem()
    emb = new_embedding()
    fp = FramePoses(data).to(DEV)
    keys = fp.keys
    code_group = {"params": list(emb.parameters()), "lr": 1e-2}
    res = {}
    if mode == "dict":
        dicts = {name: nn.ParameterDict({k: nn.Parameter(getattr(fp, name).table[i:i + 1].clone()) for i, k in enumerate(keys)})
                 for name in NAMES}
        opt = ClipAdam([{"params": list(dicts[name].parameters()), "lr": lr} for name, lr in FramePoses.LRS] + [code_group], max_norm=2.5)
        for f in SEQ:
            opt.zero_grad()
            loss = sum(quadratic(dicts[name][keys[f]], q[name]) for name in NAMES) + quadratic(emb(f)[0, :, 0, 0][None], q["code"])
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
        for name in NAMES:
            ps = list(dicts[name].values())
            zero = torch.zeros_like(ps[0])
            res[name] = {"table": torch.cat([p.detach() for p in ps]),
                         "exp_avg": torch.cat([opt.state[p]["exp_avg"] if p in opt.state else zero for p in ps]),
                         "exp_avg_sq": torch.cat([opt.state[p]["exp_avg_sq"] if p in opt.state else zero for p in ps]),
                         "step": torch.stack([opt.state[p]["step"] if p in opt.state else zero.sum() for p in ps])}
    else:
        params = [c.current for c in fp.caches] + list(emb.parameters())
        opt = ClipAdam(fp.get_parameters() + [code_group], max_norm=2.5)
        fp.attach(opt)
        frame = torch.zeros(1, dtype=torch.int32, device=DEV)

        def step(f):
            for p in params:
                p.grad = None
            fp.select(f)                                     # before the forward: it overwrites the staged parameters
            batch = {}
            fp.update(batch)
            loss = sum(quadratic(batch[k], q[name]) for k, name in zip(("Rh", "Th", "poses"), NAMES))
            loss = loss + quadratic(emb(f)[0, :, 0, 0][None], q["code"])
            loss.backward()
            opt.step()

        if mode == "eager":
            for f in SEQ:
                step(f)
        else:
            # the warm-up steps of a capture are real steps: put every tensor they touch back before the replays begin
            state = [t for c in fp.caches for t in (c.table, c.current.data, *c._opt_tables.values(), *opt.state[c.current].values())]
            state += [*fp._group.cells(), emb.frame_embs.weight.data]
            saved = [t.clone() for t in state]
            cap = CapturedStep(lambda: step(frame), params=params, slots={"frame": frame}, warmup=2)
            with torch.no_grad():
                for t, s in zip(state, saved):
                    t.copy_(s)
                for t in opt.state[emb.frame_embs.weight].values():
                    t.zero_()                                # created by the first warm-up step: a fresh optimizer's zeros
            for f in SEQ:
                cap.replay(frame=torch.tensor([f], dtype=torch.int32))
        fp.flush()
        fp.check()
        torch.cuda.synchronize()
        for c, name in zip(fp.caches, NAMES):
            res[name] = {"table": c.table.clone(), **{k: v.clone() for k, v in c.optimizer_tables().items()}}
        res["fp"], res["opt"] = fp, opt
    res["code"] = {"table": emb.frame_embs.weight.detach().clone(), **{k: v.clone() for k, v in opt.state[emb.frame_embs.weight].items()}}
    res["grad_norm"] = opt.grad_norm.clone()
    res["initial"] = {name: torch.from_numpy(np.stack([v[k] for v in data["s1"].values()])).to(DEV)
                      for name, k in zip(NAMES, ("Rh", "Th", "poses"))}
    _runs[mode] = res
    return res


def assert_same_training(a, b):
    for name in NAMES + ("code",):
        for k in ("table", "exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(a[name][k].reshape(b[name][k].shape), b[name][k]), (name, k)
    assert torch.equal(a["grad_norm"], b["grad_norm"])


def test_lazy_adam_equals_a_parameter_dict():
    """Bit equality is expected and asserted: the same optimizer kernel on the same gradient bits (the same torch expressions on
    the same values), so the fall-back bar of tests/test_gpu_optim.py:261 is not used."""
    ref, got = run("dict"), run("eager")
    assert_same_training(got, ref)
    for name in NAMES:
        assert got[name]["step"].tolist() == [2.0, 1.0, 0.0, 3.0, 1.0]
        assert torch.equal(got[name]["table"][2], got["initial"][name][2])           # never selected: untouched,
        assert not got[name]["exp_avg"][2].any() and not got[name]["exp_avg_sq"][2].any()      # no moments, step 0
        assert not torch.equal(got[name]["table"][3], got["initial"][name][3])       # the run did train
    assert float(got["grad_norm"]) > 2.5                     # and the clip was active


def test_captured_step_follows_the_frame_cell():
    """select, the code lookup, the backward and ClipAdam.step() inside ONE graph, replayed over SEQ with the frame in a device
    cell: pose tables, code table, moments and steps are the eager run's, bit for bit."""
    assert_same_training(run("captured"), run("eager"))


def test_checkpoint_round_trip():
    from d3ga_amd.frame_state import FramePoses, convert_optimizer_state
    got = run("eager")
    fp = got["fp"]
    sd = fp.state_dict()
    keys = fp.keys

    class Ref(nn.Module):
        def __init__(self):
            super().__init__()
            for name, w in zip(NAMES, (3, 3, 87)):
                setattr(self, name, nn.ParameterDict({k: nn.Parameter(torch.zeros(1, w)) for k in keys}))
    ref = Ref().to(DEV)
    ref.load_state_dict(sd, strict=True)
    fresh = FramePoses(smplx(5, 87)).to(DEV)
    fresh.load_state_dict(sd, strict=True)
    for name in NAMES:
        assert torch.equal(torch.cat(list(getattr(ref, name).values())), got[name]["table"])
        assert torch.equal(getattr(fresh, name).table, got[name]["table"])
    # the optimizer entry in the reference's layout: state for the four frames that were stepped, none for row 2
    back = convert_optimizer_state(got["opt"].state_dict(), fp.caches, to="reference")
    assert [len(g["params"]) for g in back["param_groups"]] == [5, 5, 5, 1]
    assert sorted(back["state"]) == [0, 1, 3, 4, 5, 6, 8, 9, 10, 11, 13, 14, 15]
    assert torch.equal(back["state"][13]["exp_avg"].to(DEV), got[NAMES[2]]["exp_avg"][3:4]) and float(back["state"][13]["step"]) == 3.0


# ------------------------------------------------------------------------------------------------------------------------------
# the pose-gradient chain
# ------------------------------------------------------------------------------------------------------------------------------
def rodrigues(r):
    """axis-angle (3,) -> (3,3), plain torch"""
    th = (r * r).sum().add(1e-12).sqrt()
    k = r / th
    z = torch.zeros((), device=r.device)
    K = torch.stack([torch.stack([z, -k[2], k[1]]), torch.stack([k[2], z, -k[0]]), torch.stack([-k[1], k[0], z])])
    return torch.eye(3, device=r.device) + th.sin() * K + (1 - th.cos()) * (K @ K)


def test_staged_parameters_take_the_pose_gradients():
    """FramePoses.current -> skeleton_matrices -> lbs_cage -> a scalar, on the small shapes of tests/test_gpu_lbs_pose_grad.py:
    the staged parameters receive the gradients that plain leaves holding the same values receive."""
    import os
    from d3ga_amd.cage_deform import lbs_cage, skeleton_matrices
    from d3ga_amd.frame_state import FramePoses
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lbs_pose_grad_case.npz"))
    t = lambda k: torch.from_numpy(z[k]).to(DEV)
    fp = FramePoses(smplx(4, 165)).to(DEV)
    fp.select(2)
    staged = {}
    fp.update(staged)
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in staged.items()}

    def chain(p):
        target = t("g_target_states")[:1].clone()
        target[0, :20] = target[0, :20] + 0.01 * p["poses"][0, :160].reshape(20, 8)      # 20 of the 24 joints follow the pose row
        M = skeleton_matrices(t("g_bind_state"), target)
        out = lbs_cage(t("g_vertices"), None, M[0], t("g_skin_indices"), t("g_skin_weights"), rodrigues(0.3 * p["Rh"][0]), p["Th"][0])
        return (out * t("g_grad_out")[0]).sum()

    chain(staged).backward()
    chain(leaves).backward()
    torch.cuda.synchronize()
    for k, cache in zip(("Rh", "Th", "poses"), fp.caches):
        assert cache.current.grad is not None and float(cache.current.grad.abs().max()) > 0
        assert torch.equal(cache.current.grad, leaves[k].grad), k
