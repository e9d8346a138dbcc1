"""Evaluation metrics on the device: the per-frame tail of the reference's test.py (and of train.py's progress report) --
the target composition of test.py:140-141,151, the RGBA ground truth of :186-187, `compute_errors` / `compute_heatmap` /
`dist_to_rgb` of recorder/heatmap.py:16-61, `psnr` of utils/image_utils.py:20-22 and the running means behind
errors_<trajectory>.txt (test.py:171-174,200-206) -- in three HIP launches per batch (csrc/eval.hip).  Nothing is copied to the host per frame and neither matplotlib nor torchvision is needed: the library carries
the 256-entry jet table itself.

LPIPS is a network with weights that are not part of this library: pass any callable `(fake, target) -> tensor` as `lpips`,
e.g. the reference's own `lpips.LPIPS("vgg").cuda()`; without one the third metric is NaN.

GPU tensors only (float32, contiguous), three colour channels, no gradient.  SSIM is the forward of `losses.ssim` computed by
a kernel of its own that stores one partial per tile: `d3ga_ssim_fwd` adds its workgroups' sums with float atomics, so its
last bits change from run to run, and an evaluation should print the same number twice.  Every output here is bit-reproducible.
"""
import ctypes

import torch

from . import _lib
from ._lib import D3GAError, check, require_cuda, stream_handle


class EvaluationDeviceError(D3GAError, ValueError):
    """A tensor that is not on the current GPU: a D3GAError as everywhere in this package, and a ValueError as every other
    argument error of this module."""


def _off(t, elements=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + 4 * elements)


def _bg_value(background):
    name = str(background).lower()
    if name not in ("white", "black"):
        raise ValueError(f"evaluation: background must be 'white' or 'black', got {background!r}")
    return 1.0 if name == "white" else 0.0


def _images(what, pred, image):
    """-> (B, H, W, batched) of two float32 (3,H,W) or (B,3,H,W) tensors of one shape."""
    for name, t in (("pred", pred), ("image", image)):
        if not torch.is_tensor(t):
            raise ValueError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
        if t.dim() not in (3, 4) or t.shape[-3] != 3:
            raise ValueError(f"{what}: expected {name} (3,H,W) or (B,3,H,W), got {tuple(t.shape)}")
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: {name} must be float32, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be contiguous")
    if pred.shape != image.shape:
        raise ValueError(f"{what}: pred is {tuple(pred.shape)} but image {tuple(image.shape)}")
    if pred.numel() == 0:
        raise ValueError(f"{what}: empty image {tuple(pred.shape)}")
    if image.device != pred.device:
        raise ValueError(f"{what}: image is on {image.device}, pred on {pred.device}")
    B = pred.shape[0] if pred.dim() == 4 else 1
    return B, pred.shape[-2], pred.shape[-1], pred.dim() == 4


def _device(what, *tensors):
    try:
        require_cuda(*tensors)
    except D3GAError as e:
        raise EvaluationDeviceError(f"{what}: {e}") from None


def _launch(what, pred, image, alpha, boundary_fg, bg, B, H, W, target, gt, heat, ssim, accum, channels=False):
    """The launches: pointwise, SSIM (with `ssim`), finish.  alpha None: `image` is the composed target.
    -> (metrics (B,2) [ssim, psnr], psnr_channels (B,3) or None)"""
    dev = pred.device
    flags = _lib.EVAL_BG_WHITE if bg else 0
    if alpha is None:
        flags |= _lib.EVAL_COMPOSED
    else:
        flags |= (_lib.EVAL_ALPHA3 if alpha.shape[-3] == 3 else 0) | (_lib.EVAL_BOUNDARY_F32 if boundary_fg.dtype == torch.float32 else 0)
    L = _lib.lib()
    n_part = L.d3ga_eval_partials(H, W)
    if n_part < 0:
        raise ValueError(f"{what}: a {H} x {W} frame is larger than the 2^26 pixels the evaluation kernels accept")
    if B > 65535:
        raise ValueError(f"{what}: at most 65535 frames per call, got {B}")
    with torch.no_grad():
        partials = torch.empty(B * 3 * n_part, dtype=torch.float32, device=dev)
        metrics = torch.empty(B, 2, dtype=torch.float32, device=dev)
        per_channel = torch.empty(B, 3, dtype=torch.float32, device=dev) if channels else None
        s = stream_handle()
        check(L.d3ga_eval_frames(B, H, W, flags, _off(pred), _off(image), _off(alpha), _off(boundary_fg), _off(target), _off(gt),
                                 _off(heat), _off(partials), s), "d3ga_eval_frames")
        values = None
        if ssim:
            values = torch.empty(B * L.d3ga_eval_ssim_partials(H, W), dtype=torch.float32, device=dev)
            check(L.d3ga_eval_ssim(B, H, W, _off(pred), _off(image if alpha is None else target), _off(values), s), "d3ga_eval_ssim")
        check(L.d3ga_eval_finish(B, H, W, _off(partials), _off(values), _off(metrics), _off(per_channel),
                                 None if accum is None else ctypes.c_void_p(accum.data_ptr()), s), "d3ga_eval_finish")
    return metrics, per_channel


def _composed(what, target, fake, ssim=True, channels=False):
    B, H, W, batched = _images(what, fake, target)
    _device(what, fake, target)
    heat = torch.empty_like(fake)
    metrics, per_channel = _launch(what, fake, target, None, None, 0.0, B, H, W, None, None, heat, ssim, None, channels)
    return heat, metrics, per_channel, batched


def error_heatmap(target, fake):
    """The functional form: (heatmap, ssim, psnr) of a composed target and a prediction, (3,H,W) -> a (3,H,W) heat map and two
    0-dim tensors, (B,3,H,W) -> (B,3,H,W) and two (B,) tensors.  Device tensors only; nothing is read back."""
    heat, metrics, _, batched = _composed("error_heatmap", target, fake)
    if batched:
        return heat, metrics[:, 0], metrics[:, 1]
    return heat, metrics[0, 0], metrics[0, 1]


def compute_errors(target, fake, use_npc=False, pkg=None, lpips=None):
    """recorder/heatmap.py:37-49: (heatmap (3,H,W) cuda float32, ssim, psnr, lpips), the three metrics as Python floats (ONE
    read-back for the first two).  `use_npc` and `pkg` are accepted and unused, as in the reference.  lpips: a callable
    (fake, target) -> tensor, or None (NaN)."""
    if torch.is_tensor(fake) and fake.dim() != 3:
        raise ValueError(f"compute_errors: expected (3,H,W) images, got {tuple(fake.shape)}")
    heat, metrics, _, _ = _composed("compute_errors", target, fake)
    l = float("nan") if lpips is None else float(lpips(fake, target).mean())
    s, p = metrics[0].tolist()
    return heat, s, p, l


def compute_heatmap(target, fake):
    """recorder/heatmap.py:52-61: (heat (H,W,3) float32 numpy, psnr as a Python float)."""
    if torch.is_tensor(fake) and fake.dim() != 3:
        raise ValueError(f"compute_heatmap: expected (3,H,W) images, got {tuple(fake.shape)}")
    heat, metrics, _, _ = _composed("compute_heatmap", target, fake, ssim=False)
    return heat.permute(1, 2, 0).cpu().numpy(), float(metrics[0, 1])


def psnr(img1, img2):
    """utils/image_utils.py:20-22 for (3,H,W) images: the per-channel PSNR, a (3,1) device tensor (nothing is read back)."""
    if torch.is_tensor(img1) and img1.dim() != 3:
        raise ValueError(f"psnr: expected (3,H,W) images, got {tuple(img1.shape)}")
    B, H, W, _ = _images("psnr", img1, img2)
    _device("psnr", img1, img2)
    # no output of the pointwise kernel but its partials
    _, per_channel = _launch("psnr", img1, img2, None, None, 0.0, B, H, W, None, None, None, False, None, channels=True)
    return per_channel.view(3, 1)


class Evaluator:
    """test.py's frame loop between `trainer.fit` and the PNG writers.  `add` composes the target and the RGBA ground truth,
    draws the heat map and measures SSIM and PSNR for one frame or a batch of frames, all on the device and without a
    read-back; the running sums live in a float64 device accumulator.  `summary` reads them back once; `write` writes the
    line of test.py:204-206."""

    def __init__(self, background="white", lpips=None):
        self.bg = _bg_value(background)
        self.background = str(background).lower()
        self.lpips = lpips
        self._acc = None          # [sum ssim, sum psnr, frames, sum lpips] float64, on the device of the first frame

    def reset(self):
        """Forget every frame added so far."""
        if self._acc is not None:
            self._acc.zero_()

    def add(self, pred, image, alpha, boundary_fg):
        """pred, image (3,H,W) or (B,3,H,W); alpha (1|3,H,W) or (B,1|3,H,W), channel 0 is used; boundary_fg (H,W), (1,H,W) or
        (B,1,H,W), uint8, bool or float32.  -> dict of device tensors: target and heatmap like pred, ground_truth with four
        channels, ssim and psnr 0-dim or (B,) (and lpips with a callable).  No host synchronisation."""
        what = "Evaluator.add"
        B, H, W, batched = _images(what, pred, image)
        for name, t in (("alpha", alpha), ("boundary_fg", boundary_fg)):
            if not torch.is_tensor(t):
                raise ValueError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
            if not t.is_contiguous():
                raise ValueError(f"{what}: {name} must be contiguous")
            if t.device != pred.device:
                raise ValueError(f"{what}: {name} is on {t.device}, pred on {pred.device}")
        if alpha.dtype != torch.float32:
            raise ValueError(f"{what}: alpha must be float32, got {alpha.dtype}")
        if alpha.dim() != pred.dim() or alpha.shape[-3] not in (1, 3) or alpha.shape[-2:] != pred.shape[-2:] or \
                (batched and alpha.shape[0] != B):
            raise ValueError(f"{what}: expected alpha {'(B,' if batched else '('}1|3,{H},{W}), got {tuple(alpha.shape)}")
        if boundary_fg.dtype not in (torch.uint8, torch.bool, torch.float32):
            raise ValueError(f"{what}: boundary_fg must be uint8, bool or float32, got {boundary_fg.dtype}")
        if boundary_fg.dim() < 2 or tuple(boundary_fg.shape[-2:]) != (H, W) or boundary_fg.numel() != B * H * W:
            raise ValueError(f"{what}: expected boundary_fg with {B} x {H} x {W} elements, got {tuple(boundary_fg.shape)}")
        _device(what, pred, image, alpha, boundary_fg)
        dev = pred.device
        if self._acc is None:
            self._acc = torch.zeros(4, dtype=torch.float64, device=dev)
        elif self._acc.device != dev:
            raise ValueError(f"{what}: this evaluator accumulates on {self._acc.device}, the frame is on {dev}")
        target, heat = torch.empty_like(pred), torch.empty_like(pred)
        gt = torch.empty(pred.shape[:-3] + (4, H, W), dtype=torch.float32, device=dev)
        metrics, _ = _launch(what, pred, image, alpha, boundary_fg, self.bg, B, H, W, target, gt, heat, True, self._acc)
        out = {"target": target, "ground_truth": gt, "heatmap": heat,
               "ssim": metrics[:, 0] if batched else metrics[0, 0], "psnr": metrics[:, 1] if batched else metrics[0, 1]}
        if self.lpips is not None:
            with torch.no_grad():
                if batched:
                    l = torch.stack([self.lpips(pred[b], target[b]).mean() for b in range(B)])
                else:
                    l = self.lpips(pred, target).mean()
                self._acc[3] += l.sum().double()
            out["lpips"] = l
        return out

    def summary(self):
        """{"ssim", "psnr", "lpips", "count"}: the means over the frames added since the last reset (one read-back)."""
        s, p, n, l = (0.0, 0.0, 0.0, 0.0) if self._acc is None else self._acc.tolist()
        n = int(n)
        nan = float("nan")
        if n == 0:
            return {"ssim": nan, "psnr": nan, "lpips": nan, "count": 0}
        return {"ssim": s / n, "psnr": p / n, "lpips": l / n if self.lpips is not None else nan, "count": n}

    def write(self, path):
        """test.py:200-206: `SSIM: %.5f, PSNR: %.5f, LPIPS: %.5f` into `path`; like the reference, nothing is written before
        the first frame.  -> the summary."""
        m = self.summary()
        if m["count"]:
            with open(path, "w") as f:
                f.write(f"SSIM: {m['ssim']:.5f}, ")
                f.write(f"PSNR: {m['psnr']:.5f}, ")
                f.write(f"LPIPS: {m['lpips']:.5f}\n")
        return m


def jet_table():
    """The library's 256 x 3 uint8 jet table plus the "bad" colour of a NaN error as row 256 (a CPU uint8 tensor)."""
    buf = (ctypes.c_uint8 * (257 * 3))()
    check(_lib.lib().d3ga_eval_jet_table(ctypes.cast(buf, ctypes.c_void_p)), "d3ga_eval_jet_table")
    return torch.tensor(list(buf), dtype=torch.uint8).view(257, 3)
