"""The pose prior (d3ga_amd/pose_prior.py) without a GPU: the float64 oracle against the scikit-learn golden recorded from the
reference's own build_pca / transform_pca, the g++ build of csrc/pose_prior_math.h -- the text the kernels run -- against the
oracle, first-principles answers, the host constructors and every refusal."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pose_prior_ref as R
from conftest import ROOT

NEW_EXPORTS = ("d3ga_pose_fit_scratch_bytes", "d3ga_pose_fit", "d3ga_pose_clamp")


@pytest.fixture(scope="module")
def posecheck():
    return R.posecheck()


@pytest.fixture(scope="module")
def gold():
    return R.golden()


@pytest.fixture(scope="module")
def bases(gold):
    """per golden case: the SVD oracle's basis and a PosePCA built on the host from the same rows (Gram matrix + eigh)"""
    from d3ga_amd.pose_prior import PosePCA
    out = []
    for i, (n, d, k) in enumerate(R.CASES):
        x = gold[f"c{i}_x"]
        state = {f"optimizable_poses.s_{r:05d}": torch.from_numpy(x[r:r + 1]) for r in range(n)}
        out.append((R.fit(x, k), PosePCA.from_state_dict(state, n_components=k)))
    return out


def test_fixture_is_the_recorded_one(gold):
    assert [tuple(s) for s in gold["shapes"].tolist()] == list(R.CASES) and tuple(gold["sigmas"].tolist()) == R.SIGMAS
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "pose_prior_cases.npz")) < 400 * 1024
    for i, (n, d, k) in enumerate(R.CASES):
        x, poses = R.make_case(n, d, k, seed=100 + i)
        assert np.array_equal(x, gold[f"c{i}_x"]) and np.array_equal(poses, gold[f"c{i}_poses"])
        assert gold[f"c{i}_out"].shape == (3, R.N_POSES, d) and gold[f"c{i}_clamped"].shape == (3, R.N_POSES, k)
        assert gold[f"c{i}_route"].sum() <= 0.25 * R.BAR
        if n >= 3 and k >= 2:                                # some pose has clamped and unclamped coefficients, at every sigma
            c = gold[f"c{i}_clamped"]
            assert (c.any(axis=2) & ~c.all(axis=2)).any(axis=1).all()


@pytest.mark.parametrize("case", range(len(R.CASES)))
def test_oracle_reproduces_the_scikit_learn_golden(gold, bases, case):
    n, d, k = R.CASES[case]
    basis, _ = bases[case]
    poses = gold[f"c{case}_poses"]
    v = gold[f"c{case}_variance"]
    assert np.abs(basis[2] - v).max() <= 1e-12 * v.max()
    for s, sigma in enumerate(R.SIGMAS):
        out, mask = R.clamp(basis, poses, sigma)
        ok, worst = R.within_bar(out, gold[f"c{case}_out"][s], 0.25 * R.BAR)
        assert ok, (sigma, worst)
        assert np.array_equal(mask, gold[f"c{case}_clamped"][s])
    z = R.align_signs(R.transform(basis, poses), gold[f"c{case}_z"])
    assert R.within_bar(z, gold[f"c{case}_z"], 0.25 * R.BAR)[0]
    assert R.within_bar(R.inverse_transform(basis, R.transform(basis, poses)), gold[f"c{case}_proj"], 0.25 * R.BAR)[0]


@pytest.mark.parametrize("case", range(len(R.CASES)))
def test_host_build_of_the_header_meets_the_bar(posecheck, gold, bases, case):
    """The g++ build of pose_prior_math.h with the basis PosePCA makes (covariance + eigh): every output element within
    2^-23 max|b| of the scikit-learn float64 golden and of the oracle; the float32 arithmetic of the reference is no nearer to
    exact PCA than this is to it (|ours - sk32| <= 2 |sk32 - sk64|)."""
    n, d, k = R.CASES[case]
    basis, pca = bases[case]
    x, poses = gold[f"c{case}_x"], gold[f"c{case}_poses"]
    mean, cov = R.host_fit(posecheck, x)
    m0, c0 = R.covariance(x)
    assert np.abs(mean - m0).max() <= 1e-12 * max(np.abs(m0).max(), 1e-300) and np.abs(cov - c0).max() <= 1e-12 * np.abs(c0).max()
    assert np.array_equal(cov, cov.T)
    assert pca.n_components_ == k and pca.components_.shape == (k, d)
    assert np.abs(pca.explained_variance_ - gold[f"c{case}_variance"]).max() <= 1e-10 * gold[f"c{case}_variance"].max()
    for s, sigma in enumerate(R.SIGMAS):
        got = R.host_clamp(posecheck, pca, poses, sigma)
        assert got.dtype == np.float32 and got.shape == (R.N_POSES, d)
        sk64, sk32 = gold[f"c{case}_out"][s], gold[f"c{case}_out32"][s]
        for want in (sk64, R.clamp(basis, poses, sigma)[0]):
            ok, worst = R.within_bar(got, want)
            assert ok, (sigma, worst)
        assert np.abs(got - sk32).max() <= 2.0 * np.abs(sk32 - sk64).max(), (sigma, np.abs(got - sk32).max(), np.abs(sk32 - sk64).max())
    z = R.host_clamp(posecheck, pca, poses, 0.0, stages=1)
    assert z.shape == (R.N_POSES, k) and R.within_bar(R.align_signs(z.astype(np.float64), gold[f"c{case}_z"]), gold[f"c{case}_z"])[0]
    back = R.host_clamp(posecheck, pca, z, 0.0, stages=4)
    assert back.shape == (R.N_POSES, d)
    # z went through float32: its rounding, 2^-24 |z|, comes back through orthonormal components
    bound = R.BAR * np.abs(gold[f"c{case}_proj"]).max() + 2.0 ** -24 * np.abs(gold[f"c{case}_z"]).max() * np.sqrt(k)
    assert np.abs(back - gold[f"c{case}_proj"]).max() <= bound


def test_first_principles(posecheck, gold, bases):
    for case in (2, 4):                                      # (9, 8, 8): k = D; (33, 87, 30)
        n, d, k = R.CASES[case]
        basis, pca = bases[case]
        poses = gold[f"c{case}_poses"]
        mean32 = pca.mean_.astype(np.float32)
        # a pose equal to the mean returns the mean (the float32 mean is within 2^-24 of it, and so is what comes back)
        got = R.host_clamp(posecheck, pca, mean32, 2.0)
        assert R.within_bar(got[0], pca.mean_)[0]
        # sigma = 0 returns the mean, exactly rounded
        got = R.host_clamp(posecheck, pca, poses, 0.0)
        assert np.array_equal(got, np.broadcast_to(mean32, got.shape))
        # a very large sigma returns the projection onto the subspace
        got = R.host_clamp(posecheck, pca, poses, 1e30)
        proj = R.inverse_transform(basis, R.transform(basis, poses))
        assert R.within_bar(got, proj)[0]
        if k == d:                                           # ... which is the pose itself, within the store rounding
            assert R.within_bar(got, poses)[0]
        # the sign of a component does not matter
        flipped = type(pca).from_arrays(pca.mean_, -pca.components_, pca.explained_variance_)
        a, b = R.host_clamp(posecheck, pca, poses, 2.0), R.host_clamp(posecheck, flipped, poses, 2.0)
        assert R.within_bar(a, b.astype(np.float64), 2.0 ** -24)[0]
    # a NaN in the pose comes out as NaN, an infinite sigma clips nothing
    basis, pca = bases[3]
    bad = gold["c3_poses"][:1].copy()
    bad[0, 2] = np.nan
    assert np.isnan(R.host_clamp(posecheck, pca, bad, 2.0)).all()
    assert np.array_equal(R.host_clamp(posecheck, pca, gold["c3_poses"], float("inf")), R.host_clamp(posecheck, pca, gold["c3_poses"], 1e30))


def test_sign_rule_and_variance_floor():
    from d3ga_amd.pose_prior import PosePCA, _decompose
    rng = np.random.default_rng(0)
    x = rng.standard_normal((40, 6)) * np.array([3.0, 2.0, 1.0, 0.5, 0.0, 0.0])     # two columns without variance
    mean, cov = R.covariance(x)
    comp, var = _decompose(mean, cov, 6)
    assert (var >= 0).all() and (np.diff(var) <= 0).all() and var[4] <= 1e-12
    lead = np.abs(comp).argmax(axis=1)
    assert (comp[np.arange(6), lead] > 0).all()
    np.testing.assert_allclose(comp @ comp.T, np.eye(6), atol=1e-12)
    with pytest.raises(ValueError, match="not finite"):
        _decompose(mean, cov * np.nan, 3)
    state = {f"optimizable_poses.a_{i:05d}": torch.from_numpy(x[i:i + 1]).float() for i in range(40)}
    a, b = PosePCA.from_state_dict(state, 4), PosePCA.from_state_dict(state, 4)
    assert np.array_equal(a.components_, b.components_)


def test_value_errors():
    from d3ga_amd.pose_prior import PosePCA
    cpu = torch.zeros(10, 8)
    with pytest.raises(ValueError, match="at least two"):
        PosePCA.fit(torch.zeros(1, 8), 1)
    with pytest.raises(ValueError, match="1..256"):
        PosePCA.fit(torch.zeros(10, 257), 1)
    with pytest.raises(ValueError, match="1..256"):
        PosePCA.fit(torch.zeros(10, 0), 1)
    for k in (0, 9, 11):
        with pytest.raises(ValueError, match=r"n_components=.* must be between 1 and min\(n_samples, n_features\)=8"):
            PosePCA.fit(cpu, k)
    with pytest.raises(ValueError, match="min"):
        PosePCA.fit(torch.zeros(3, 8), 4)                    # scikit-learn's own rule: k <= min(N, D)
    with pytest.raises(ValueError, match=r"\(N,D\)"):
        PosePCA.fit(torch.zeros(8), 1)
    with pytest.raises(ValueError, match="GPU only"):
        PosePCA.fit(cpu, 3)
    with pytest.raises(ValueError, match="do not fit"):
        PosePCA.from_arrays(np.zeros(4), np.zeros((2, 5)), np.ones(2))
    with pytest.raises(ValueError, match="finite"):
        PosePCA.from_arrays(np.zeros(4), np.full((2, 4), np.nan), np.ones(2))
    pca = PosePCA.from_arrays(np.zeros(4), np.eye(4)[:2], np.ones(2))
    with pytest.raises(ValueError, match="GPU only"):
        pca.clamp(torch.zeros(4))
    with pytest.raises(ValueError, match=r"\(4,\)"):
        pca.clamp(torch.zeros(5))
    with pytest.raises(ValueError, match="sigma"):
        pca.clamp(torch.zeros(4), sigma=-1.0)
    with pytest.raises(ValueError, match="int32"):
        pca.clamp_rows(torch.zeros(3, 4), torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match="table"):
        pca.clamp_rows(torch.zeros(3, 5), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="GPU only"):
        pca.clamp_rows(torch.zeros(3, 4), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="GPU only"):
        pca.transform(torch.zeros(2, 4))
    with pytest.raises(ValueError, match="GPU only"):
        pca.inverse_transform(torch.zeros(2, 2))
    pca.check()                                              # nothing was ever launched
    with pytest.raises((AttributeError, ValueError)):
        pca.mean_[0] = 1.0                                   # read-only
    # the C ABI refuses the same before any launch (the pointers are never read)
    from d3ga_amd import _lib
    L = _lib.lib()
    one, nb = ctypes.c_void_p(256), ctypes.c_int64()
    assert L.d3ga_pose_fit_scratch_bytes(1, 8, ctypes.byref(nb)) == -2 and L.d3ga_pose_fit_scratch_bytes(8, 257, ctypes.byref(nb)) == -2
    assert L.d3ga_pose_fit_scratch_bytes(8, 8, None) == -1
    assert L.d3ga_pose_fit_scratch_bytes(257, 165, ctypes.byref(nb)) == 0 and nb.value == 2 * (165 + 165 * 165) * 8
    assert L.d3ga_pose_fit(one, 1, 8, one, one, None) == -2 and L.d3ga_pose_fit(None, 4, 8, one, one, None) == -1
    assert L.d3ga_pose_fit(one, 4, 8, one, ctypes.c_void_p(260), None) == -3
    clamp = lambda **kw: L.d3ga_pose_clamp(*[kw.get(n, v) for n, v in (("inp", one), ("rows", None), ("n_rows", 0), ("B", 1), ("D", 8),
                                                                          ("k", 3), ("mean", one), ("comp", one), ("comp_t", one), ("std", one),
                                                                          ("sigma", 2.0), ("stages", 7), ("out", one), ("flag", None),
                                                                          ("stream", None))])
    assert clamp(B=0) == -2 and clamp(D=257) == -2 and clamp(k=0) == -2 and clamp(k=257) == -2
    assert clamp(stages=3) == -3 and clamp(stages=0) == -3 and clamp(stages=8) == -3 and clamp(sigma=float("nan")) == -3
    assert clamp(inp=None) == -1 and clamp(out=None) == -1 and clamp(std=None) == -1
    assert clamp(rows=one, n_rows=4) == -1                   # rows without a flag
    assert clamp(rows=one, n_rows=0, flag=one) == -2 and clamp(rows=one, n_rows=4, flag=one, stages=4) == -3
    assert clamp(comp=ctypes.c_void_p(260)) == -3


def test_host_constructors_and_round_trip(gold, bases, posecheck):
    from d3ga_amd.pose_prior import PosePCA
    assert PosePCA.from_state_dict({"frame_embs.weight": torch.zeros(3, 4)}) is None and PosePCA.from_state_dict({}) is None
    x = gold["c3_x"]                                         # (90, 8, 3)
    state = {"embeddings.frame_embs.weight": torch.zeros(90, 32)}
    order = [5, 0, 17] + [r for r in range(90) if r not in (5, 0, 17)]              # dictionary order, not key order
    for r in order:
        state[f"model.optimizable_poses.seq_{r:05d}"] = torch.from_numpy(x[r:r + 1])
        state[f"model.optimizable_rotations.seq_{r:05d}"] = torch.zeros(1, 3)
    pca = PosePCA.from_state_dict(state, n_components=3)
    basis = R.fit(x, 3)
    assert pca.n_components_ == 3 and pca.mean_.dtype == np.float64
    assert np.abs(pca.mean_ - basis[0]).max() <= 1e-13 and np.abs(pca.explained_variance_ - basis[2]).max() <= 1e-12 * basis[2].max()
    assert np.abs(np.abs(np.sum(pca.components_ * basis[1], axis=1)) - 1.0).max() <= 1e-9
    with pytest.raises(ValueError, match="n_components=15"):
        PosePCA.from_state_dict(state)                       # the default of build_pca_pillow needs 15 <= min(N, D)

    class Fitted:                                            # what an unpickled sklearn PCA looks like from here
        mean_, components_, explained_variance_ = basis[0].astype(np.float32), basis[1].tolist(), basis[2]
    sk = PosePCA.from_sklearn(Fitted)
    assert sk.components_.dtype == np.float64 and np.array_equal(sk.components_, basis[1])
    poses = gold["c3_poses"]
    got = R.host_clamp(posecheck, PosePCA.from_arrays(*basis), poses, 2.0)
    assert R.within_bar(got, gold["c3_out"][1])[0]
    # state_dict / load_state_dict
    sd = pca.state_dict()
    assert set(sd) == {"mean", "components", "explained_variance"} and all(v.dtype == torch.float64 for v in sd.values())
    other = PosePCA.from_arrays(np.zeros(2), np.eye(2), np.ones(2)).load_state_dict(sd)
    assert np.array_equal(other.mean_, pca.mean_) and np.array_equal(other.components_, pca.components_)
    assert np.array_equal(other.explained_variance_, pca.explained_variance_) and other.n_components_ == 3
    assert np.array_equal(R.host_clamp(posecheck, other, poses, 2.0), R.host_clamp(posecheck, pca, poses, 2.0))


def test_abi_lists_the_new_entry_points():
    import d3ga_amd
    from d3ga_amd import _lib, pose_prior
    from d3ga_amd.csrc import build as b
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "d3ga.h")).read(), flags=re.S)
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS and re.search(r"\bint\s+%s\s*\(" % name, src), name
    assert "pose_prior.hip" in b.SOURCES and "pose_prior_math.h" in b.HEADERS and "-ffp-contract=off" in b.EXTRA["pose_prior.hip"]
    assert _lib.ABI_VERSION == 112 and re.search(r"#define\s+D3GA_VERSION\s+112\b", src) and _lib.lib().d3ga_version() == 112
    for n in ("POSE_MAX_D", "POSE_FIT_CHUNK", "POSE_STAGE_PROJECT", "POSE_STAGE_CLIP", "POSE_STAGE_RECONSTRUCT"):
        assert getattr(_lib, n) == int(re.search(r"#define\s+D3GA_%s\s+(\d+)" % n, src).group(1)), n
    assert pose_prior.FIT_CHUNK == _lib.POSE_FIT_CHUNK and pose_prior.MAX_D == _lib.POSE_MAX_D
    assert "PosePCA" in d3ga_amd.__all__ and d3ga_amd.PosePCA is pose_prior.PosePCA
