"""Frame state (d3ga_amd/frame_state.py) without a GPU: the float64 restatement against the fixture of the reference's Embedding,
the key order and checkpoint layout of FramePoses, the optimizer-state conversion against a real lazily stepped torch.optim.Adam,
and every refusal."""
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

import frame_state_ref as R
from conftest import GOLDEN, ROOT

NEW_EXPORTS = ("d3ga_code_lookup_fwd", "d3ga_code_lookup_bwd", "d3ga_table_mean_scratch_bytes", "d3ga_table_mean",
               "d3ga_row_cache_select", "d3ga_row_cache_flush")


def cases():
    z = np.load(os.path.join(GOLDEN, "frame_state_cases.npz"))
    return [{k: z[f"c{i}_{k}"] for k in ("n", "d", "idx", "max_norm", "before", "after", "out", "dout", "dweight", "average")}
            for i in range(int(z["n_cases"]))]


def smplx(n_frames=5, width=87, seqs=("s1",)):
    g = np.random.default_rng(7)
    return {s: {3 * i + 1: {"Rh": g.normal(size=3).astype(np.float32), "Th": g.normal(size=3).astype(np.float32),
                            "poses": g.normal(size=width).astype(np.float32), "expression": np.zeros(10, np.float32)}
                for i in range(n_frames)} for s in seqs}


def test_restatement_reproduces_the_fixture():
    """float64 against the reference's float32: 4 eps on a scaled element (the norm's sum, the square root, the scale and the
    product, each rounded), the gradient sums and the mean of at most seven terms likewise"""
    cs = cases()
    assert len(cs) == 7 and {(int(c["n"]), int(c["d"])) for c in cs[:6]} == {(n, d) for n in (1, 7) for d in (1, 5, 32)}
    for i, c in enumerate(cs):
        n, mx = int(c["n"]), float(c["max_norm"])
        assert mx == float(c["d"]) and (c["idx"] >= n).any() and len(set(np.clip(c["idx"], 0, n - 1))) < len(c["idx"])
        norms = np.sqrt((c["before"].astype(np.float64) ** 2).sum(1))
        if i < 6:                                            # (the constructed case sits ON the threshold on purpose)
            assert (np.abs(norms - mx) > 1e-3 * mx).all()
        after, out = R.code_lookup_fwd(c["before"], c["idx"], mx)
        np.testing.assert_allclose(after, c["after"], rtol=5e-7, atol=0)
        np.testing.assert_allclose(out, c["out"], rtol=5e-7, atol=0)
        rows = set(R.clamp_rows(c["idx"], n).tolist())
        for r in range(n):
            if r not in rows or norms[r] <= mx:
                assert np.array_equal(c["after"][r], c["before"][r])
            else:
                assert not np.array_equal(c["after"][r], c["before"][r])
        dw = R.code_lookup_bwd(c["dout"], c["idx"], n)
        np.testing.assert_allclose(dw, c["dweight"], rtol=5e-7, atol=1e-7)
        assert not c["dweight"][[r for r in range(n) if r not in rows]].any()
        np.testing.assert_allclose(R.table_mean(c["before"]), c["average"], rtol=0, atol=5e-7 * np.abs(c["before"]).max())
    last = cs[-1]
    assert np.array_equal(last["after"][0], [3, 4, 0, 0, 0]) and np.array_equal(last["after"][1], [3, 4, 0, 0, 0])


def test_row_cache_model_is_a_write_back_cache():
    t = np.arange(12.0).reshape(4, 3)
    s = np.zeros((1, 3))
    m = R.RowCacheModel([(t, s)])
    m.select(2); s += 100
    m.select(2)
    assert np.array_equal(t[2], [6, 7, 8]) and np.array_equal(s[0], [106, 107, 108])
    m.select(0)
    assert np.array_equal(t[2], [106, 107, 108]) and np.array_equal(s[0], [0, 1, 2]) and m.prev == 0
    m.select(4); m.select(-1)
    assert m.flag == 1 and m.prev == 0 and np.array_equal(s[0], [0, 1, 2])
    s += 1
    m.flush(); m.flush()
    assert np.array_equal(t[0], [1, 2, 3]) and m.prev == 0


def test_frame_poses_keys_and_checkpoint_layout():
    from d3ga_amd.frame_state import FramePoses, RowCache
    data = smplx(5, 87)
    fp = FramePoses(data)
    keys = [f"s1_{str(3 * i + 1).zfill(5)}" for i in range(5)]
    assert fp.keys == keys == fp.optimizable_rotations.keys == fp.optimizable_translations.keys
    assert [fp.index(k) for k in keys] == list(range(5)) and fp.optimizable_poses.index("s1_00007") == 2
    assert [(n, tuple(p.shape)) for n, p in fp.named_parameters()] == [("optimizable_rotations.current", (1, 3)),
                                                                       ("optimizable_translations.current", (1, 3)),
                                                                       ("optimizable_poses.current", (1, 87))]
    assert [(g["lr"], len(g["params"])) for g in fp.get_parameters()] == [(0.001, 1), (0.0001, 1), (0.001, 1)]
    sd = fp.state_dict()
    assert list(sd) == [f"{d}.{k}" for d in ("optimizable_rotations", "optimizable_translations", "optimizable_poses") for k in keys]
    assert all(tuple(v.shape) == ((1, 87) if "poses" in k else (1, 3)) for k, v in sd.items())
    assert np.array_equal(sd["optimizable_poses.s1_00007"].numpy()[0], data["s1"][7]["poses"])
    assert np.array_equal(sd["optimizable_translations.s1_00013"].numpy()[0], data["s1"][13]["Th"])

    # the reference's module: three ParameterDicts (models/garment_net.py:104-106), both directions with strict=True
    class Ref(nn.Module):
        def __init__(self):
            super().__init__()
            for name, w in (("optimizable_rotations", 3), ("optimizable_translations", 3), ("optimizable_poses", 87)):
                setattr(self, name, nn.ParameterDict({k: nn.Parameter(torch.zeros(1, w)) for k in keys}))
    ref = Ref()
    ref.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in ref.state_dict().items())
    with torch.no_grad():
        for p in ref.parameters():
            p.add_(1.0)
    fp2 = FramePoses(smplx(5, 87))
    fp2.load_state_dict(ref.state_dict(), strict=True)
    assert all(torch.equal(v, sd[k] + 1.0) for k, v in fp2.state_dict().items())
    bad = dict(ref.state_dict())
    bad["optimizable_poses.s1_99999"] = torch.zeros(1, 87)
    del bad["optimizable_rotations.s1_00001"]
    with pytest.raises(RuntimeError, match="s1_99999"):
        fp2.load_state_dict(bad, strict=True)
    # several sequences: all of them are registered (the reference keeps the last one only)
    assert len(FramePoses(smplx(2, 165, seqs=("a", "b"))).keys) == 4
    assert RowCache({"x": torch.zeros(1, 4), "y": torch.ones(1, 4)}).state_dict()["y"].shape == (1, 4)


def test_convert_optimizer_state_against_a_lazily_stepped_adam():
    """A ParameterDict of five entries stepped over [0, 3, 3, 1]: only the picked entry has a gradient, so torch's Adam leaves
    rows 2 and 4 without state; row 3 has step 2."""
    from d3ga_amd.frame_state import RowCache, convert_optimizer_state
    g = torch.Generator().manual_seed(3)
    entries = {f"k{i}": torch.randn(1, 6, generator=g) for i in range(5)}
    pd = nn.ParameterDict({k: nn.Parameter(v.clone()) for k, v in entries.items()})
    other = nn.Parameter(torch.randn(4, generator=g))
    opt = torch.optim.Adam([{"params": list(pd.parameters()), "lr": 1e-3}, {"params": [other], "lr": 1e-2}])
    for f in (0, 3, 3, 1):
        opt.zero_grad()
        (pd[f"k{f}"].square().sum() + other.sum()).backward()
        opt.step()
    sd = opt.state_dict()
    assert sorted(sd["state"]) == [0, 1, 3, 5]
    cache = RowCache(entries)
    new, tables = convert_optimizer_state(sd, [cache], to="tables")
    (t,) = tables
    assert t["step"].tolist() == [1.0, 1.0, 0.0, 2.0, 0.0]
    for r in (2, 4):
        assert not t["exp_avg"][r].any() and not t["exp_avg_sq"][r].any()
    for r, pid in ((0, 0), (1, 1), (3, 3)):
        assert torch.equal(t["exp_avg"][r], sd["state"][pid]["exp_avg"][0]) and torch.equal(t["exp_avg_sq"][r], sd["state"][pid]["exp_avg_sq"][0])
    assert [g_["params"] for g_ in new["param_groups"]] == [[0], [1]] and new["param_groups"][1]["lr"] == 1e-2
    assert float(new["state"][0]["step"]) == 0.0 and tuple(new["state"][0]["exp_avg"].shape) == (1, 6)
    assert torch.equal(new["state"][1]["exp_avg"], sd["state"][5]["exp_avg"])
    # the tables layout loads into an optimizer over the staged parameter ...
    opt2 = torch.optim.Adam([{"params": [cache.current], "lr": 1e-3}, {"params": [nn.Parameter(other.detach().clone())], "lr": 1e-2}])
    opt2.load_state_dict(new)
    # ... and back: the reference's layout again, state for the stepped entries only
    back = convert_optimizer_state(opt2.state_dict(), [cache], to="reference", tables=tables)
    assert sorted(back["state"]) == [0, 1, 3, 5] and [g_["params"] for g_ in back["param_groups"]] == [[0, 1, 2, 3, 4], [5]]
    for pid in (0, 1, 3, 5):
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(back["state"][pid][k], sd["state"][pid][k]), (pid, k)
        assert float(back["state"][pid]["step"]) == float(sd["state"][pid]["step"])
    opt3 = torch.optim.Adam([{"params": [nn.Parameter(v.clone()) for v in entries.values()], "lr": 1e-3}, {"params": [nn.Parameter(other.detach().clone())], "lr": 1e-2}])
    opt3.load_state_dict(back)
    with pytest.raises(ValueError):
        convert_optimizer_state(new, [cache], to="tables")           # one parameter where five are expected
    with pytest.raises(ValueError):
        convert_optimizer_state(sd, [cache], to="sideways")


def test_refusals():
    import d3ga_amd
    from d3ga_amd import _lib
    from d3ga_amd.frame_state import Embedding, FramePoses, RowCache, code_lookup
    emb = Embedding(9, 4, height=2, width=3)
    assert tuple(emb.frame_embs.weight.shape) == (9, 24) and emb.max_norm == 4.0 and list(emb.state_dict()) == ["frame_embs.weight"]
    with pytest.raises(ValueError, match="at most 16"):
        emb(torch.zeros(17, dtype=torch.long))                       # B > 16: before anything touches a device
    with pytest.raises(ValueError):
        code_lookup(torch.zeros(3, 4097), 0)                         # D > 4096
    with pytest.raises(d3ga_amd.D3GAError):
        emb(torch.zeros(2, dtype=torch.long))                        # a CPU forward
    with pytest.raises(d3ga_amd.D3GAError):
        emb.average()
    with pytest.raises(TypeError):
        code_lookup(emb.frame_embs.weight, torch.zeros(2))
    fp = FramePoses(smplx(3, 87))
    for batch in ([0, 1], torch.tensor([0, 1]), (2, 2)):
        with pytest.raises(ValueError, match="one row is staged"):
            fp.select(batch)
        with pytest.raises(ValueError, match="one row is staged"):
            fp.optimizable_poses.select(batch)
    with pytest.raises(IndexError):
        fp.select(3)
    with pytest.raises(IndexError):
        fp.select(-1)
    with pytest.raises(KeyError):
        fp.select("s1_00002")
    with pytest.raises(d3ga_amd.D3GAError):
        fp.select(1)                                                 # rows on the CPU
    with pytest.raises(ValueError, match="host"):
        fp.attach(torch.optim.Adam(fp.get_parameters()))             # Adam with a host `step`
    with pytest.raises(ValueError, match="not a parameter"):
        fp.attach(torch.optim.Adam([nn.Parameter(torch.zeros(2))], capturable=True))
    with pytest.raises(ValueError):
        RowCache({"a": torch.zeros(1, 3), "b": torch.zeros(1, 4)})
    # the C ABI refuses the same sizes (no launch is made: the pointers are never read)
    L = _lib.lib()
    one = _lib.ctypes.c_void_p(256)
    assert L.d3ga_code_lookup_fwd(one, one, 4, 8, 17, 1.0, one, None) == -2
    assert L.d3ga_code_lookup_fwd(one, one, 4, 4097, 1, 1.0, one, None) == -2
    assert L.d3ga_code_lookup_bwd(one, one, 0, 8, 1, one, None) == -2
    assert L.d3ga_code_lookup_fwd(None, one, 4, 8, 1, 1.0, one, None) == -1
    assert L.d3ga_table_mean(one, 0, 8, one, one, None) == -2 and L.d3ga_table_mean(one, 4, 8, one, _lib.ctypes.c_void_p(4), None) == -3
    pairs = (_lib.RowPair * 17)(*[_lib.RowPair(256, 256, 3, 5)] * 17)
    assert L.d3ga_row_cache_select(pairs, 17, one, one, one, None) == -2 and L.d3ga_row_cache_select(pairs, 0, one, one, one, None) == -2
    assert L.d3ga_row_cache_flush(pairs, 2, None, one, None) == -1
    need = _lib.ctypes.c_int64()
    assert L.d3ga_table_mean_scratch_bytes(20000, 32, _lib.ctypes.byref(need)) == 0 and need.value == 64 * 32 * 8


def test_abi_lists_the_new_entry_points():
    import d3ga_amd
    from d3ga_amd import _lib
    from d3ga_amd.csrc import build as b
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "d3ga.h")).read(), flags=re.S)
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS and re.search(r"\bint\s+%s\s*\(" % name, src), name
    assert "frame_state.hip" in b.SOURCES
    assert (_lib.CODE_MAX_B, _lib.CODE_MAX_D, _lib.ROW_CACHE_MAX_PAIRS) == tuple(
        int(re.search(r"#define\s+D3GA_%s\s+(\d+)" % n, src).group(1)) for n in ("CODE_MAX_B", "CODE_MAX_D", "ROW_CACHE_MAX_PAIRS"))
    assert _lib.ctypes.sizeof(_lib.RowPair) == 24
    assert {"code_lookup", "Embedding", "RowCache", "FramePoses", "convert_optimizer_state"} <= set(d3ga_amd.__all__)
