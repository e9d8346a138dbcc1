"""The training objective (d3ga_amd/objective.py) without a GPU: the float64 restatement against the reference's own
scale_energy in the deform fixtures, its float32 form, known answers of the assembly, the g++ build of csrc/objective_math.h
-- the text the kernels run -- against the restatement, and every refusal."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import objective_ref as R
from conftest import GOLDEN, ROOT

NEW_EXPORTS = ("d3ga_scale_energy_fwd", "d3ga_scale_energy_bwd", "d3ga_objective_fwd", "d3ga_objective_bwd")
W = R.WEIGHTS


@pytest.fixture(scope="module")
def objcheck():
    return R.objcheck()


def _golden(name):
    z = np.load(os.path.join(GOLDEN, name))
    return torch.from_numpy(z["scaling_param"]), torch.from_numpy(z["d_scale"]), z["scale_energy"]


@pytest.mark.parametrize("name,P", [("deform_case0.npz", 257), ("deform_case1.npz", 1000)])
def test_restatement_reproduces_the_reference_scale_energy(name, P):
    """float64 against the reference's float32 mean of 3P squares: a few 2^-24 (measured 3e-8 relative)"""
    scaling, d_scale, want = _golden(name)
    assert tuple(scaling.shape) == (P, 3) and want.shape == (1,) and want.dtype == np.float32
    got = R.scale_energy(scaling, d_scale)
    assert tuple(got.shape) == (1,)
    assert abs(float(got) - float(want[0])) <= 2e-7 * float(want[0])
    # the activated scales the fixture holds are the ones the restatement squares
    z = np.load(os.path.join(GOLDEN, name))
    np.testing.assert_allclose(torch.exp(scaling + d_scale).numpy(), z["scales"], rtol=2e-6)


def test_float32_and_float64_restatements_agree():
    for name in ("deform_case0.npz", "deform_case1.npz"):
        scaling, d_scale, _ = _golden(name)
        a, b = R.scale_energy(scaling, d_scale, dtype=torch.float32), R.scale_energy(scaling, d_scale)
        assert a.dtype == torch.float32 and abs(float(a) - float(b)) <= 1e-6 * float(b)
        a, b = R.scale_energy(scaling, None, "none", torch.float32), R.scale_energy(scaling, None, "none")
        assert abs(float(a) - float(b)) <= 1e-6 * float(b)
    for B, kw in ((1, {}), (4, dict(n_cages=3, D=300)), (2, dict(fm=False, blur=False, vgg=False, poses=0))):
        frames = R.make_frames(B, seed=3, **kw)
        t32, l32 = R.objective(frames, W, torch.float32)
        t64, l64 = R.objective(frames, W)
        assert list(l32) == list(R.KEY_ORDER)
        for k in R.KEY_ORDER:
            assert abs(float(l32[k]) - float(l64[k])) <= 1e-5 * abs(float(l64[k])), k


def test_known_answers_of_the_assembly(objcheck):
    zeros = lambda: {"l1": torch.zeros(()), "ssim": torch.zeros(()), "sil_l1": torch.zeros(()), "scale_energy": torch.zeros(3),
                     "fm_energy": torch.zeros(3), "frame_encoding": torch.zeros(32), "optimizable_poses": torch.zeros(1, 87),
                     "blur_weights": None, "vgg": torch.zeros(())}
    want = W["lambda_dssim"] * W["rgb_weight"] + 3.0 * W["fme_weight"]
    total, losses = R.objective([zeros()], W)
    assert abs(float(total) - want) < 1e-12
    terms, _ = R.host_forward(objcheck, [zeros()], W)
    assert abs(float(terms[8]) - want) <= 2e-7 * want and terms[6] == 0.0 and terms[4] == 0.0
    # one frame against two identical frames
    fr = R.make_frames(1, n_cages=3, seed=5)[0]
    assert abs(float(R.objective([fr], W)[0]) - float(R.objective([fr, dict(fr)], W)[0])) < 1e-12
    t1, _ = R.host_forward(objcheck, [fr], W)
    t2, _ = R.host_forward(objcheck, [fr, dict(fr)], W)
    np.testing.assert_allclose(t1, t2, rtol=3e-7, atol=0)
    # each weight scales exactly its own term
    base = R.objective([fr], W)[1]
    hbase, _ = R.host_forward(objcheck, [fr], W)
    for wname, term in (("rgb_weight", "color_loss"), ("sil_weight", "sil_loss"), ("fme_weight", "fme_loss"), ("blur_weight", "blur_loss"),
                        ("vgg_weight", "vgg_loss")):
        w2 = dict(W, **{wname: 2.0 * W[wname]})
        l2 = R.objective([fr], w2)[1]
        h2, _ = R.host_forward(objcheck, [fr], w2)
        for i, k in enumerate(R.KEY_ORDER[:-1]):
            ratio = 2.0 if k == term else 1.0
            assert abs(float(l2[k]) - ratio * float(base[k])) <= 1e-12, (wname, k)
            assert h2[i] == np.float32(ratio) * hbase[i], (wname, k)                  # a power of two: exact in float32
        assert abs((float(l2["total_loss"]) - float(base["total_loss"])) - float(base[term])) <= 1e-12
    lam = R.objective([fr], dict(W, lambda_dssim=1.0))[1]["color_loss"]
    assert abs(float(lam) - (1.0 - float(fr["ssim"])) * W["rgb_weight"]) < 1e-12


@pytest.mark.parametrize("B,kw", [(1, {}), (2, dict(n_cages=3, D=1)), (4, dict(n_cages=3, D=300)), (3, dict(fm=False, poses=0)),
                                  (1, dict(blur=False, vgg=False)), (16, dict(n_cages=16, D=4096, poses=165))])
def test_host_build_of_the_header_equals_the_restatement(objcheck, B, kw):
    """Forward: relative 1e-5 on every term (the derived bound is < 100 * 2^-24 at the limits).  Gradients: the
    project's rule on every element."""
    frames = R.make_frames(B, seed=11, requires_grad=True, **kw)
    total, losses = R.objective(frames, W)
    terms, status = R.host_forward(objcheck, frames, W)
    for i, k in enumerate(R.KEY_ORDER):
        want = float(losses[k].detach())
        assert abs(float(terms[i]) - want) <= R.FWD_RTOL * abs(want), (k, terms[i], want)
    assert status[:3].tolist() == [0, 0, 1]
    total.backward()
    got = R.host_backward(objcheck, frames, W)
    lv = R.leaves(frames)
    assert len(lv) == len(got)
    for f, k, t in lv:
        assert R.grad_close(torch.from_numpy(got[(f, k)]), t.grad.reshape(-1)), (f, k)


def test_host_status_words_and_scale_energy_terms(objcheck):
    frames = R.make_frames(1, seed=2)
    status = np.zeros(16, np.int32)
    R.host_forward(objcheck, frames, W, status)
    bad = [dict(frames[0], l1=torch.tensor(float("inf")))]
    terms, _ = R.host_forward(objcheck, bad, W, status)
    assert np.isinf(terms[8]) and status[:3].tolist() == [0, 0, 2]                    # an infinite total is not flagged
    enc = frames[0]["frame_encoding"].clone()
    enc[7] = float("nan")
    terms, _ = R.host_forward(objcheck, [dict(frames[0], frame_encoding=enc)], W, status)
    assert status[:3].tolist() == [1, 2, 3] and np.isnan(terms[7]) and np.isnan(terms[8])
    kept = status[4:13].view(np.float32).copy()
    assert np.array_equal(kept, terms, equal_nan=True) and np.isfinite(kept[0])
    R.host_forward(objcheck, frames, W, status)                                       # later finite steps do not clear it
    R.host_forward(objcheck, [dict(frames[0], l1=torch.tensor(float("nan")))], W, status)
    assert status[:3].tolist() == [1, 2, 5] and np.array_equal(status[4:13].view(np.float32), kept, equal_nan=True)
    # scale_energy's per-element functions against the reference's value, and the underflowing square
    for name in ("deform_case0.npz", "deform_case1.npz"):
        scaling, d_scale, want = _golden(name)
        a, b = scaling.numpy().reshape(-1), d_scale.numpy().reshape(-1)
        grad = np.empty_like(a)
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        e = objcheck.hc_scale_energy(ctypes.c_int64(a.size), p(a), p(b), 1, ctypes.c_float(1.0), p(grad))
        assert abs(e - float(want[0])) <= 1e-6 * float(want[0])
        s = scaling.double().requires_grad_(True)
        R.scale_energy(s, d_scale).backward()
        assert R.grad_close(torch.from_numpy(grad), s.grad.reshape(-1))
    x = np.full(6, -60.0, np.float32)
    grad = np.full(6, np.nan, np.float32)
    assert objcheck.hc_scale_energy(ctypes.c_int64(6), p(x), None, 1, ctypes.c_float(1.0), p(grad)) == 0.0 and not grad.any()


def test_refusals():
    from d3ga_amd import _lib
    from d3ga_amd.objective import TrainingObjective, scale_energy
    obj = TrainingObjective(**W)
    assert TrainingObjective.from_config(W).weights == obj.weights == TrainingObjective.from_config(type("T", (), W)).weights
    fr = lambda **kw: dict(R.make_frames(1, n_cages=3, seed=1)[0], **kw)
    with pytest.raises(ValueError, match="frame_encoding"):
        obj([fr(frame_encoding=None)])
    with pytest.raises(ValueError, match="same ones"):
        obj([fr(), fr(vgg=None)])                                        # frames with different sets of optional keys
    with pytest.raises(ValueError, match="same ones"):
        obj([fr(fm_energy=None), fr()])
    with pytest.raises(ValueError, match="cages"):
        obj([fr(), fr(scale_energy=torch.zeros(2))])                     # mismatched n_cages
    with pytest.raises(ValueError, match="cages"):
        obj([fr(), fr(fm_energy=torch.zeros(4))])
    with pytest.raises(ValueError, match="GPU only"):
        obj([fr()])                                                      # CPU tensors
    with pytest.raises(ValueError, match="one element"):
        obj([fr(l1=torch.zeros(2))])
    with pytest.raises(ValueError, match="4096"):
        obj([fr(frame_encoding=torch.zeros(4097))])
    with pytest.raises(ValueError):
        obj([])
    with pytest.raises(ValueError):
        obj([fr()] * 17)
    with pytest.raises(ValueError, match="has not been called"):
        obj.report()
    obj.check(), obj.poll()                                              # nothing was ever launched: nothing to report
    assert obj.status() == {"nan_seen": False, "first_bad_step": None, "steps": 0}
    with pytest.raises(ValueError, match="GPU only"):
        scale_energy(torch.zeros(5, 3))
    with pytest.raises(ValueError, match="activation"):
        scale_energy(torch.zeros(5, 3), activation="softplus")
    with pytest.raises(ValueError, match="differ"):
        scale_energy(torch.zeros(5, 3), torch.zeros(4, 3))
    # the C ABI refuses the same (no launch is made: the pointers are never read)
    L = _lib.lib()
    one = ctypes.c_void_p(256)
    assert L.d3ga_scale_energy_fwd(0, one, None, 1, one, one, None) == -2
    assert L.d3ga_scale_energy_fwd(8, None, None, 1, one, one, None) == -1
    assert L.d3ga_scale_energy_fwd(8, one, None, 2, one, one, None) == -3
    assert L.d3ga_scale_energy_fwd(8, ctypes.c_void_p(260), None, 1, one, one, None) == -3
    assert L.d3ga_scale_energy_bwd(8, one, ctypes.c_void_p(260), 1, one, one, None) == -3

    def desc(n_frames=1, skip=(), lens=None, goff=-1):
        d = _lib.ObjectiveDesc()
        d.n_frames = n_frames
        for f in range(min(max(n_frames, 0), _lib.OBJ_MAX_FRAMES)):
            for slot, n in enumerate((1, 1, 1, 3, 3, 32, 87, 3, 1)):
                if (f, slot) in skip:
                    continue
                e = d.entry[f * 9 + slot]
                e.ptr, e.len, e.goff = 256, (lens or {}).get((f, slot), n), goff
        return d
    assert L.d3ga_objective_fwd(None, one, one, None) == -1
    assert L.d3ga_objective_fwd(desc(0), one, one, None) == -2 and L.d3ga_objective_fwd(desc(17), one, one, None) == -2
    assert L.d3ga_objective_fwd(desc(1, skip={(0, 5)}), one, one, None) == -1          # no frame_encoding
    assert L.d3ga_objective_fwd(desc(2, skip={(1, 8)}), one, one, None) == -3          # different optional entries
    assert L.d3ga_objective_fwd(desc(2, lens={(1, 3): 2}), one, one, None) == -3       # mismatched n_cages
    assert L.d3ga_objective_fwd(desc(1, lens={(0, 5): 4097}), one, one, None) == -2
    assert L.d3ga_objective_fwd(desc(1, lens={(0, 0): 2}), one, one, None) == -2
    assert L.d3ga_objective_fwd(desc(1), None, one, None) == -1
    assert L.d3ga_objective_bwd(desc(1, goff=100), one, one, 131, None) == -2          # an entry reaching outside the buffer
    assert L.d3ga_objective_bwd(desc(1), one, one, 0, None) == 0                       # nothing wants a gradient: no launch


def test_abi_lists_the_new_entry_points():
    import d3ga_amd
    from d3ga_amd import _lib
    from d3ga_amd.csrc import build as b
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "d3ga.h")).read(), flags=re.S)
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS and re.search(r"\bint\s+%s\s*\(" % name, src), name
    assert "objective.hip" in b.SOURCES and "objective_math.h" in b.HEADERS and "-ffp-contract=off" in b.EXTRA["objective.hip"]
    assert _lib.ABI_VERSION == 112 and re.search(r"#define\s+D3GA_VERSION\s+112\b", src) and _lib.lib().d3ga_version() == 112
    names = ("SCALE_ACT_NONE", "SCALE_ACT_EXP", "SCALE_ENERGY_GRID", "OBJ_MAX_FRAMES", "OBJ_SLOTS", "OBJ_MAX_LEN", "OBJ_TERMS",
             "OBJ_STATUS_NAN_SEEN", "OBJ_STATUS_FIRST_BAD", "OBJ_STATUS_STEPS", "OBJ_STATUS_TERMS", "OBJ_STATUS_WORDS")
    for n in names:
        assert getattr(_lib, n) == int(re.search(r"#define\s+D3GA_%s\s+(\d+)" % n, src).group(1)), n
    assert _lib.SCALE_ENERGY_GRID <= _lib.LOSS_PARTIALS
    assert ctypes.sizeof(_lib.ObjectiveEntry) == 16 and ctypes.sizeof(_lib.ObjectiveDesc) == 32 + 16 * 9 * 16 == ctypes.sizeof(R.Desc)
    assert ctypes.sizeof(_lib.ObjectiveDesc) <= 4096                                  # it travels in the kernel arguments
    assert {"scale_energy", "TrainingObjective"} <= set(d3ga_amd.__all__)
    assert d3ga_amd.TrainingObjective.KEY_ORDER == R.KEY_ORDER and d3ga_amd.TrainingObjective.KEYS == R.KEYS
