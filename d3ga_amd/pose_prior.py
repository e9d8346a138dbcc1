"""The pose prior (csrc/pose_prior.hip): the PCA over the refined poses that the reference builds once per
run, and the clamp that every driven frame goes through before its pose conditions the field networks.

Drop-ins for
    test.py:264-274  build_pca_pillow      PosePCA.fit(fp.optimizable_poses.table, 30)   (or PosePCA.from_state_dict)
    test.py:49-56    transform_pca         pca.clamp(poses, sigma=2.0)
    test.py:88-92    the per-frame detour  pca.clamp_rows(table, cell, sigma=2.0, out=lbs_slot)   (capturable)
The fit's sums (float64 mean and covariance) and the clamp run on the GPU; the eigen-solve of the (D,D) covariance, D <= 256,
once per run, is numpy.linalg.eigh on the host.  The other constructors never touch the GPU.

    fp.flush()
    pca = PosePCA.fit(fp.optimizable_poses.table, n_components=30)
    lbs = torch.empty(1, 87, device="cuda")
    with torch.cuda.graph(g):
        pca.clamp_rows(drive_poses, frame_cell, sigma=2.0, out=lbs)        # frame_cell: (1,) int32 on the device
    ...
    pca.check()                                                            # IndexError if a replay named a row outside the table
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, dptr, stream_handle

__all__ = ["PosePCA", "FIT_CHUNK", "MAX_D"]

FIT_CHUNK = _lib.POSE_FIT_CHUNK      # rows per reduction chunk of the fit, whatever the launch looks like
MAX_D = _lib.POSE_MAX_D              # widest pose and most components
_CLAMP = _lib.POSE_STAGE_PROJECT | _lib.POSE_STAGE_CLIP | _lib.POSE_STAGE_RECONSTRUCT


def _on_gpu(what, *tensors):
    """ValueError for anything that is not a tensor on the current GPU (there is no CPU fallback)."""
    cur = None
    for t in tensors:
        if t is None:
            continue
        if not torch.is_tensor(t):
            raise ValueError(f"{what}: expected a tensor, got {type(t).__name__}")
        if not t.is_cuda:
            raise ValueError(f"{what}: runs on the GPU only (tensor on {t.device}); there is no CPU fallback")
        if cur is None:
            cur = torch.cuda.current_device()
        if t.device.index != cur:
            raise ValueError(f"{what}: tensor on {t.device} but the current device is cuda:{cur} (launches go to the current "
                             f"device's stream)")


def _check_fit_shape(what, n, d, k):
    if n < 2:
        raise ValueError(f"{what}: {n} poses, a covariance needs at least two")
    if not 1 <= d <= MAX_D:
        raise ValueError(f"{what}: poses of {d} values, expected 1..{MAX_D}")
    if not 1 <= k <= min(n, d):
        raise ValueError(f"{what}: n_components={k} must be between 1 and min(n_samples, n_features)={min(n, d)}")


def _decompose(mean, cov, k):
    """The k largest eigenpairs of a float64 covariance in descending order -> (components (k,D), variance (k,)).
    var_j = max(lambda_j, 0); every component gets the sign that makes its largest-magnitude entry positive."""
    if not (np.isfinite(cov).all() and np.isfinite(mean).all()):
        raise ValueError("PosePCA: the mean or the covariance of the poses is not finite")
    lam, vec = np.linalg.eigh(cov)                           # ascending
    lam, vec = lam[::-1][:k], vec[:, ::-1][:, :k]
    comp = np.ascontiguousarray(vec.T)
    lead = np.abs(comp).argmax(axis=1)
    sign = np.where(comp[np.arange(k), lead] < 0, -1.0, 1.0)
    return comp * sign[:, None], np.maximum(lam, 0.0)


class PosePCA:
    """PCA(n_components).fit(poses) of scikit-learn (full solver, no whitening) and the reference's transform_pca.

    mean_ (D,), components_ (k,D), explained_variance_ (k,), n_components_: read-only float64 numpy, as scikit-learn names them
    (a component's sign is this class's own rule; the clamp does not depend on it).

    clamp(x, sigma) for a pose x (D), all float64 until the one rounding of the result to float32:
        z_j = sum_d (x_d - mean_d) V_jd;  zc_j = min(max(z_j, -sigma std_j), sigma std_j);  out_d = (sum_j zc_j V_jd) + mean_d
    with std = sqrt(explained_variance_).  A NaN in the pose comes out as NaN."""

    def __init__(self, mean, components, explained_variance):
        mean = np.array(mean, dtype=np.float64).reshape(-1)
        comp = np.array(components, dtype=np.float64)
        var = np.array(explained_variance, dtype=np.float64).reshape(-1)
        if comp.ndim != 2 or comp.shape[1] != mean.shape[0] or var.shape[0] != comp.shape[0]:
            raise ValueError(f"PosePCA: mean {mean.shape}, components {comp.shape} and explained_variance {var.shape} do not fit "
                             "(D,), (k,D), (k,)")
        k, d = comp.shape
        if not 1 <= d <= MAX_D or not 1 <= k <= MAX_D:
            raise ValueError(f"PosePCA: components {comp.shape}, expected 1..{MAX_D} of 1..{MAX_D} values")
        if not (np.isfinite(mean).all() and np.isfinite(comp).all() and np.isfinite(var).all()):
            raise ValueError("PosePCA: mean, components and explained_variance must be finite")
        self._mean, self._comp, self._var = mean, np.ascontiguousarray(comp), var
        for a in (self._mean, self._comp, self._var):
            a.setflags(write=False)
        self.covariance_ = None                              # (D,D) float64 as the device summed it: set by fit() only
        self._dev = None

    # ---- constructors ------------------------------------------------------------------------------------------------------
    @classmethod
    def fit(cls, poses, n_components):
        """poses: (N,D) float32 on the GPU, e.g. `fp.optimizable_poses.table` after `fp.flush()`; it is read where it is.
        2 <= N, 1 <= D <= 256, 1 <= n_components <= min(N, D) (scikit-learn's rule), else ValueError.  Four launches leave the
        float64 mean and covariance in one buffer; ONE read-back of D + D*D doubles (the only synchronisation) hands them to
        numpy.linalg.eigh.  Two fits of the same table are equal bit for bit."""
        if not torch.is_tensor(poses) or poses.dim() != 2:
            raise ValueError(f"PosePCA.fit: expected poses (N,D), got {tuple(poses.shape) if torch.is_tensor(poses) else type(poses).__name__}")
        n, d = poses.shape
        k = int(n_components)
        _check_fit_shape("PosePCA.fit", n, d, k)
        if n * d > 2**31 - 1:
            raise ValueError(f"PosePCA.fit: a table of {n} x {d} is beyond the kernels' 32-bit indices")
        _on_gpu("PosePCA.fit", poses)
        if poses.dtype != torch.float32:
            raise ValueError(f"PosePCA.fit: poses must be float32, got {poses.dtype}")
        src = poses.detach().contiguous()
        need = ctypes.c_int64()
        check(_lib.lib().d3ga_pose_fit_scratch_bytes(n, d, ctypes.byref(need)), "d3ga_pose_fit_scratch_bytes")
        scratch = torch.empty(need.value // 8, dtype=torch.float64, device=src.device)
        out = torch.empty(d + d * d, dtype=torch.float64, device=src.device)
        check(_lib.lib().d3ga_pose_fit(dptr(src), n, d, dptr(out), dptr(scratch), stream_handle()), "d3ga_pose_fit")
        host = out.cpu().numpy()                             # the one synchronisation
        mean, cov = host[:d].copy(), host[d:].reshape(d, d).copy()
        self = cls(mean, *_decompose(mean, cov, k))
        self.covariance_ = cov
        self._upload(src.device)
        return self

    @classmethod
    def from_arrays(cls, mean, components, explained_variance):
        return cls(mean, components, explained_variance)

    @classmethod
    def from_sklearn(cls, obj):
        """obj: anything with mean_, components_ and explained_variance_ (a fitted sklearn PCA the caller has unpickled)."""
        return cls(obj.mean_, obj.components_, obj.explained_variance_)

    @classmethod
    def from_state_dict(cls, model_state, n_components=15):
        """build_pca_pillow (test.py:264-274) on the host: every entry whose key contains "optimizable_poses", in dictionary
        order, row [0] of each; None when there is none.  Centre, covariance and eigen-solve in float64 numpy."""
        rows = []
        for key, value in model_state.items():
            if "optimizable_poses" in key:
                v = value.detach().cpu().numpy() if torch.is_tensor(value) else np.asarray(value)
                rows.append(np.asarray(v[0], dtype=np.float64).reshape(-1))
        if len(rows) == 0:
            return None
        x = np.stack(rows)
        n, d = x.shape
        k = int(n_components)
        _check_fit_shape("PosePCA.from_state_dict", n, d, k)
        mean = x.mean(axis=0)
        xc = x - mean
        cov = xc.T @ xc / (n - 1)
        return cls(mean, *_decompose(mean, cov, k))

    # ---- the basis ---------------------------------------------------------------------------------------------------------
    mean_ = property(lambda self: self._mean)
    components_ = property(lambda self: self._comp)
    explained_variance_ = property(lambda self: self._var)
    n_components_ = property(lambda self: self._comp.shape[0])
    n_features_ = property(lambda self: self._comp.shape[1])

    def state_dict(self):
        return {"mean": torch.from_numpy(self._mean.copy()), "components": torch.from_numpy(self._comp.copy()),
                "explained_variance": torch.from_numpy(self._var.copy())}

    def load_state_dict(self, state):
        get = lambda k: state[k].detach().cpu().numpy() if torch.is_tensor(state[k]) else state[k]
        other = PosePCA(get("mean"), get("components"), get("explained_variance"))
        self._mean, self._comp, self._var, self._dev = other._mean, other._comp, other._var, None
        return self

    def _upload(self, device):
        """mean (D), components (k,D), their transpose (D,k) and std (k) as float64 on the device, and the flag cell."""
        if self._dev is None or self._dev["device"] != device:
            up = lambda a: torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(device)
            self._dev = {"device": device, "mean": up(self._mean), "comp": up(self._comp), "comp_t": up(self._comp.T),
                         "std": up(np.sqrt(np.maximum(self._var, 0.0))), "flag": torch.zeros(1, dtype=torch.int32, device=device)}
        return self._dev

    # ---- the per-frame path ------------------------------------------------------------------------------------------------
    def _launch(self, what, src, rows, n_rows, b, sigma, stages, out, shape):
        k, d = self._comp.shape
        width = d if stages & _lib.POSE_STAGE_RECONSTRUCT else k
        _on_gpu(what, src, rows, out)
        dev = self._upload(src.device)
        if out is None:
            out = torch.empty(shape if shape is not None else (b, width), dtype=torch.float32, device=src.device)
        elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != b * width:
            raise ValueError(f"{what}: out must be contiguous float32 with {b} x {width} elements, got {out.dtype} {tuple(out.shape)}")
        check(_lib.lib().d3ga_pose_clamp(dptr(src), dptr(rows), n_rows, b, d, k, dptr(dev["mean"]), dptr(dev["comp"]),
                                         dptr(dev["comp_t"]), dptr(dev["std"]), float(sigma), stages, dptr(out), dptr(dev["flag"]),
                                         stream_handle()), "d3ga_pose_clamp")
        return out

    def _rows_of(self, what, x, width):
        """x (width,), (1,width) or (B,width) -> (contiguous float32 (B,width), B)"""
        if not torch.is_tensor(x) or x.dim() not in (1, 2) or x.shape[-1] != width or x.numel() == 0:
            raise ValueError(f"{what}: expected ({width},) or (B,{width}), got {tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.float().contiguous()                       # (a copy: hand over contiguous float32 to avoid it)
        return x, x.numel() // width

    def clamp(self, x, sigma=3.0, out=None):
        """transform_pca (test.py:49-56) of x (D,), (1,D) or (B,D) -> the same shape, float32, in ONE launch whatever B is.
        sigma: the reference's default; test.py passes 2.0.  With `out` (contiguous float32 of the same size) and x contiguous
        float32 nothing is allocated and nothing synchronises: capturable."""
        x, b = self._rows_of("PosePCA.clamp", x, self._comp.shape[1])
        return self._launch("PosePCA.clamp", x, None, 0, b, self._sigma(sigma), _CLAMP, out, x.shape)

    def clamp_rows(self, table, rows, sigma=3.0, out=None):
        """clamp(table[rows]) without the gather: table (N,D) float32, rows an int32 device tensor of B >= 1 row indices that
        the KERNEL reads -- a (1,) cell is the form a captured step follows from replay to replay -> (B,D).  A row outside
        [0, N) leaves its output row untouched and sets a sticky device flag: see check()."""
        d = self._comp.shape[1]
        if not torch.is_tensor(table) or table.dim() != 2 or table.shape[1] != d or table.shape[0] < 1:
            raise ValueError(f"PosePCA.clamp_rows: expected table (N,{d}), got {tuple(table.shape) if torch.is_tensor(table) else type(table).__name__}")
        if table.dtype != torch.float32 or not table.is_contiguous():
            raise ValueError("PosePCA.clamp_rows: table must be contiguous float32 (it is read where it is)")
        if not torch.is_tensor(rows) or rows.dtype != torch.int32 or rows.numel() < 1 or not rows.is_contiguous():
            raise ValueError("PosePCA.clamp_rows: rows must be a contiguous int32 device tensor of at least one index")
        return self._launch("PosePCA.clamp_rows", table.detach(), rows, table.shape[0], rows.numel(), self._sigma(sigma), _CLAMP, out, None)

    def transform(self, x):
        """PCA.transform: x (D,) or (B,D) -> (B,k) float32 coefficients, not clipped"""
        x, b = self._rows_of("PosePCA.transform", x, self._comp.shape[1])
        return self._launch("PosePCA.transform", x, None, 0, b, 0.0, _lib.POSE_STAGE_PROJECT, None, None)

    def inverse_transform(self, z):
        """PCA.inverse_transform: z (k,) or (B,k) -> (B,D) float32"""
        z, b = self._rows_of("PosePCA.inverse_transform", z, self._comp.shape[0])
        return self._launch("PosePCA.inverse_transform", z, None, 0, b, 0.0, _lib.POSE_STAGE_RECONSTRUCT, None, None)

    @staticmethod
    def _sigma(sigma):
        sigma = float(sigma)
        if sigma != sigma or sigma < 0:
            raise ValueError(f"PosePCA: sigma={sigma}, expected a number >= 0")
        return sigma

    def check(self):
        """Raises IndexError if a clamp_rows since the start (or a replay of a captured one) was given a row outside its table.
        Reads one device word: synchronises."""
        if self._dev is not None and int(self._dev["flag"]) != 0:
            raise IndexError("PosePCA.clamp_rows: a call was given a row outside its table: nothing was written for it, and the "
                             "output row kept what it held before")
