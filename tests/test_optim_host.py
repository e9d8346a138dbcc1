"""ClipAdam without a GPU: the float64 oracle (tests/optim_ref.py) against the reference's optimizer (clip_grad_norm_ +
torch.optim.Adam on float64 CPU tensors), the chunk-table builder as a pure host function, the new ABI surface and the
constructor's refusals."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from optim_ref import clip_adam_step_ref, gradient_scale

NEW_EXPORTS = ("d3ga_optim_scratch_bytes", "d3ga_optim_clip_adam_step")


def test_oracle_equals_clip_grad_norm_and_torch_adam_in_float64():
    gen = torch.Generator().manual_seed(11)
    sizes = [(7,), (33, 5), (1,), (4097,), (16, 16, 3)]
    lrs = [1e-3, 5e-4, 1e-2, 1.6e-4, 2.5e-3]
    params = [torch.nn.Parameter(torch.randn(s, generator=gen, dtype=torch.float64)) for s in sizes]
    opt = torch.optim.Adam([{"params": [p], "lr": lr} for p, lr in zip(params, lrs)], betas=(0.9, 0.999), eps=1e-8)
    P = [p.detach().clone() for p in params]
    M, V, S = [torch.zeros_like(p) for p in P], [torch.zeros_like(p) for p in P], [0] * 5
    n_clipped = 0
    for it in range(100):
        grads = [gradient_scale(it, i) * torch.randn(s, generator=gen, dtype=torch.float64) for i, s in enumerate(sizes)]
        if it % 4 == 3:
            grads[2] = None                                     # torch's skip rule: this tensor takes no part in the step
        for p, g in zip(params, grads):
            p.grad = None if g is None else g.clone()
        norm_t = torch.nn.utils.clip_grad_norm_(params, 2.5, foreach=True)
        opt.step()
        P, M, V, S, norm = clip_adam_step_ref(P, grads, M, V, S, lrs, [(0.9, 0.999)] * 5, [1e-8] * 5, 2.5)
        assert abs(float(norm) - float(norm_t)) <= 1e-13 * float(norm_t), (it, float(norm), float(norm_t))
        n_clipped += float(norm) > 2.5
        for i, (p, q) in enumerate(zip(params, P)):
            err = (p.detach() - q).abs()
            assert bool((err <= 1e-12 * (1.0 + q.abs())).all()), (it, i, float(err.max()))
    assert n_clipped == 50                                      # every other step is far above the threshold, the rest far below
    assert S == [100, 100, 75, 100, 100]
    assert [int(opt.state[p]["step"]) for p in params] == S


def test_plan_builder_chunks_tails_alignment_and_key():
    from d3ga_amd import _lib, optim
    C = _lib.OPTIM_CHUNK
    assert C % 4 == 0 and optim.CHUNK_DTYPE.itemsize == 48 and optim.TENSOR_DTYPE.itemsize == 16
    assert [optim.n_chunks_of(n) for n in (1, C - 1, C, C + 1, 3 * C, 3 * C + 5)] == [1, 1, 1, 2, 3, 4]
    base = 0x7F0000000000
    #          p             g                 m                 v                 numel      step          group
    entries = [(base, base + 0x100000, base + 0x200000, base + 0x300000, 3 * C + 5, base + 0x900000, 0),
               (base + 0x400000, base + 0x500000, base + 0x600000, base + 0x700000, 1, base + 0x900010, 2),
               (base + 0x800004, base + 0xA00000, base + 0xB00000, base + 0xC00000, C, base + 0x900020, 1)]    # p: a view 4 bytes in
    table, tensors = optim.build_plan(entries)
    assert table.dtype == optim.CHUNK_DTYPE and len(table) == 4 + 1 + 1 and len(tensors) == 3
    assert table["n"].tolist() == [C, C, C, 5, 1, C]            # whole chunks, then what remains
    assert int(table["n"].sum()) == sum(e[4] for e in entries)
    assert table["tensor"].tolist() == [0, 0, 0, 0, 1, 2]
    for name, col in (("p", 0), ("g", 1), ("m", 2), ("v", 3)):
        assert table[name][:4].tolist() == [entries[0][col] + 4 * C * k for k in range(4)]
        assert int(table[name][4]) == entries[1][col] and int(table[name][5]) == entries[2][col]
    assert table["flags"].tolist() == [_lib.OPTIM_ALIGNED16] * 5 + [0]          # the offset view takes the element-wise path
    assert tensors["step"].tolist() == [e[5] for e in entries] and tensors["group"].tolist() == [0, 2, 1]
    assert not table["reserved"].any() and not tensors["reserved"].any()
    # a misaligned gradient alone is enough to drop the flag
    t2, _ = optim.build_plan([(base, base + 8, base + 0x200000, base + 0x300000, 10, base + 0x900000, 0)])
    assert t2["flags"].tolist() == [0] and t2["n"].tolist() == [10]
    with pytest.raises(ValueError):
        optim.build_plan([(base, base, base, base, 0, base, 0)])
    # the key: unchanged when nothing moves, changed when one gradient does
    live = [(e[0], e[1], e[4], e[6]) for e in entries]
    assert optim.plan_key(live) == optim.plan_key(list(live))
    moved = list(live)
    moved[1] = (live[1][0], live[1][1] + 512, live[1][2], live[1][3])
    assert optim.plan_key(moved) != optim.plan_key(live)
    assert optim.plan_key(live[:2]) != optim.plan_key(live)     # a gradient that is None this step


def test_new_abi_surface():
    import ctypes
    from d3ga_amd import _lib
    src = open(os.path.join(ROOT, "include", "d3ga.h")).read()
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert hasattr(_lib.lib(), name)
    assert _lib.ABI_VERSION == 112 and re.search(r"#define\s+D3GA_VERSION\s+112\b", src)
    assert _lib.OPTIM_CHUNK == int(re.search(r"#define\s+D3GA_OPTIM_CHUNK\s+(\d+)", src).group(1))
    assert _lib.OPTIM_ALIGNED16 == int(re.search(r"#define\s+D3GA_OPTIM_ALIGNED16\s+(\d+)", src).group(1))
    L = _lib.lib()
    out = ctypes.c_int64()
    assert L.d3ga_optim_scratch_bytes(3418, 60, 5, ctypes.byref(out)) == 0
    assert out.value >= 4 * 3418 + 4 + 32 * 60 and out.value % 256 == 0
    assert L.d3ga_optim_scratch_bytes(-1, 1, 1, ctypes.byref(out)) == -2        # D3GA_E_SIZE
    assert L.d3ga_optim_scratch_bytes(1, 1, 1, None) == -1                       # D3GA_E_NULL
    assert L.d3ga_optim_clip_adam_step(None, 1, None, 1, None, 1, 2.5, None, None, None) == -1
    one = ctypes.c_void_p(256)                                                   # (never dereferenced: the sizes are refused first)
    assert L.d3ga_optim_clip_adam_step(one, 0, one, 1, one, 1, 2.5, one, None, None) == -2
    assert L.d3ga_optim_clip_adam_step(one, 1, one, 2, one, 1, 2.5, one, None, None) == -2    # more tensors than chunks


def test_constructor_refusals():
    from d3ga_amd import D3GAError
    from d3ga_amd.optim import ClipAdam
    p = lambda *a, **k: torch.nn.Parameter(torch.zeros(*(a or (4,)), **k))
    for kw, word in ((dict(amsgrad=True), "amsgrad"), (dict(maximize=True), "maximize"), (dict(weight_decay=1e-4), "weight_decay"),
                     (dict(differentiable=True), "differentiable"), (dict(max_norm=-1.0), "max_norm"), (dict(lr=-1.0), "lr"),
                     (dict(betas=(0.9, 1.0)), "betas"), (dict(eps=-1.0), "eps")):
        with pytest.raises(ValueError, match=word):
            ClipAdam([p()], **kw)
    with pytest.raises(ValueError, match="amsgrad"):                     # also as a per-group option
        ClipAdam([{"params": [p()], "amsgrad": True}])
    with pytest.raises(ValueError, match="float32"):
        ClipAdam([p(dtype=torch.float64)])
    with pytest.raises(ValueError, match="float32"):
        ClipAdam([p(dtype=torch.bfloat16)])
    with pytest.raises(ValueError, match="contiguous"):
        ClipAdam([torch.nn.Parameter(torch.zeros(4, 6).t())])
    with pytest.raises(ValueError, match="more than one device"):
        ClipAdam([p(), p(device="meta")])
    with pytest.raises(D3GAError, match="no CPU fallback"):              # never a ValueError: a RuntimeError of this package
        ClipAdam([p()], lr=1e-3, max_norm=2.5)
    with pytest.raises(D3GAError):
        ClipAdam(params=[{"params": [p()], "lr": 1e-4}, {"params": [p(3, 3)], "lr": 1e-3}], max_norm=2.5)    # utils/load_module.py:20-26
