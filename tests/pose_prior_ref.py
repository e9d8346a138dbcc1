"""Float64 numpy oracle of the pose prior (d3ga_amd/pose_prior.py) in the project's own words, the data
of its tests, and the g++ build of csrc/pose_prior_math.h (tests/hostcheck/posecheck.cpp) -- the text the kernels run."""
import ctypes
import os
import subprocess

import numpy as np

from conftest import GOLDEN, ROOT

BAR = 2.0 ** -23                 # |a - b| <= BAR * max|b| per output element (DESIGN.md 4.4n has the derivation)
CASES = ((2, 3, 1), (5, 1, 1), (9, 8, 8), (90, 8, 3), (33, 87, 30), (150, 87, 30), (257, 165, 100))      # (N, D, k)
SIGMAS = (1.5, 2.0, 3.0)
N_POSES = 5


# ---- the oracle --------------------------------------------------------------------------------------------------------------
def fit(x, k):
    """centre, SVD, S^2 / (N - 1) -> (mean (D,), components (k,D), variance (k,)), all float64"""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    mean = x.mean(axis=0)
    _, s, vt = np.linalg.svd(x - mean, full_matrices=False)
    return mean, vt[:k].copy(), (s[:k] ** 2) / (n - 1)


def covariance(x):
    x = np.asarray(x, dtype=np.float64)
    mean = x.mean(axis=0)
    xc = x - mean
    return mean, xc.T @ xc / (x.shape[0] - 1)


def transform(basis, x):
    mean, comp, _ = basis
    return (np.asarray(x, dtype=np.float64).reshape(-1, mean.shape[0]) - mean) @ comp.T


def inverse_transform(basis, z):
    mean, comp, _ = basis
    return np.asarray(z, dtype=np.float64).reshape(-1, comp.shape[0]) @ comp + mean


def clamp(basis, x, sigma):
    """clip, back-project -> (B,D) float64; and the mask of the clamped coefficients (B,k)"""
    z = transform(basis, x)
    lim = sigma * np.sqrt(basis[2])
    zc = np.minimum(np.maximum(z, -lim), lim)
    return inverse_transform(basis, zc), zc != z


def within_bar(a, b, bar=BAR):
    """every element of a within bar * max|b| of b -> (ok, the largest difference as a share of max|b|)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = float(np.abs(b).max())
    worst = float(np.abs(a - b).max())
    return worst <= bar * scale, (worst / scale if scale > 0 else worst)


# ---- data --------------------------------------------------------------------------------------------------------------------
def make_case(n, d, k, seed, n_poses=N_POSES):
    """X = (G diag(s)) Q + c with s_j = r^min(j, k+1), r = max(0.6, 1e-4^(1/k)): the kept components have a separated spectrum.
    Poses: X[b] + (3 g s) Q.  Both float32, as the device takes them."""
    rng = np.random.default_rng(seed)
    r = max(0.6, 1e-4 ** (1.0 / k))
    s = r ** np.minimum(np.arange(d), k + 1)
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    c = rng.standard_normal(d)
    x = (rng.standard_normal((n, d)) * s) @ q + c
    poses = x[np.arange(n_poses) % n] + (3.0 * rng.standard_normal((n_poses, d)) * s) @ q
    return x.astype(np.float32), poses.astype(np.float32)


def golden():
    return np.load(os.path.join(GOLDEN, "pose_prior_cases.npz"), allow_pickle=False)


def align_signs(z_mine, z_ref):
    """z_mine with every column given the sign z_ref has in the row where |z_ref| of that column is largest"""
    row = np.abs(z_ref).argmax(axis=0)
    cols = np.arange(z_ref.shape[1])
    s = np.where(z_mine[row, cols] * z_ref[row, cols] < 0, -1.0, 1.0)
    return z_mine * s


# ---- the g++ build of pose_prior_math.h --------------------------------------------------------------------------------------
def posecheck():
    src = os.path.join(ROOT, "tests", "hostcheck", "posecheck.cpp")
    out_dir = os.path.join(ROOT, "tests", "hostcheck", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libposecheck.so")
    deps = [src, os.path.join(ROOT, "d3ga_amd", "csrc", "pose_prior_math.h"), os.path.join(ROOT, "include", "d3ga.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", so])
    return ctypes.CDLL(so)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_fit(lib, x):
    """(mean (D,), covariance (D,D)) of a float32 table by the header's chunked sums"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, d = x.shape
    out = np.zeros(d + d * d, np.float64)
    assert lib.hc_pose_fit(_p(x), n, d, _p(out)) == 0
    return out[:d].copy(), out[d:].reshape(d, d).copy()


def host_clamp(lib, pca, x, sigma, stages=7):
    """The header's clamp with the basis of a PosePCA (or anything with mean_, components_, explained_variance_) -> float32"""
    mean = np.ascontiguousarray(pca.mean_, dtype=np.float64)
    comp = np.ascontiguousarray(pca.components_, dtype=np.float64)
    comp_t = np.ascontiguousarray(comp.T)
    std = np.sqrt(np.maximum(np.asarray(pca.explained_variance_, dtype=np.float64), 0.0))
    k, d = comp.shape
    w_in, w_out = (d if stages & 1 else k), (d if stages & 4 else k)
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1, w_in))
    out = np.zeros((x.shape[0], w_out), np.float32)
    st = lib.hc_pose_clamp(_p(x), x.shape[0], d, k, _p(mean), _p(comp), _p(comp_t), _p(std), ctypes.c_double(sigma), stages, _p(out))
    assert st == 0, st
    return out
