"""Image tail of the Goliath configuration (configs/goliath_axe184.yml: use_blur), between render() and the losses.

Drop-ins for the reference's
    models/learnable_blur.py  LearnableBlur              (models/garment_net.py:20,45; models/trainer.py:124-126)
    train.py:182-188          target / silhouette target (compose_target)
each one HIP launch per direction (csrc/image_tail.hip).  GPU tensors only; every op runs inside graph.CapturedStep.
The Gaussian taps, the sigma rule and the reflect padding are torchvision's `gaussian_blur`, restated from memory
(DESIGN.md sec. 2).
"""
import copy

import torch
from torch import nn

from . import _lib
from ._lib import check, dptr, f32c16, require_cuda, stream_handle

_cam_cells = {}


def _cam_cell(cam_idx, n_cameras, device):
    """cam_idx as the (1,) int32 device tensor the kernels read.  A host integer is validated here and served from a small
    per-device table (no host-to-device copy per call); a device tensor is the caller's -- the kernels clamp it."""
    if torch.is_tensor(cam_idx):
        if cam_idx.dtype != torch.int32 or cam_idx.numel() != 1 or not cam_idx.is_cuda:
            raise ValueError("learnable_blur: cam_idx must be an int or a (1,) int32 tensor on the GPU")
        require_cuda(cam_idx)
        return cam_idx
    i = int(cam_idx)
    if not 0 <= i < n_cameras:
        raise IndexError(f"learnable_blur: camera index {i} outside [0, {n_cameras})")
    key = (device.index, i)
    if key not in _cam_cells:
        _cam_cells[key] = torch.tensor([i], dtype=torch.int32, device=device)
    return _cam_cells[key]


class _BlurMix(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, weights_raw, cell):
        require_cuda(img, weights_raw)
        x = f32c16(img)
        wr = f32c16(weights_raw)
        if x.dim() != 3 or wr.dim() != 2 or wr.shape[1] != 3:
            raise ValueError(f"learnable_blur: expected img (C,H,W) and weights_raw (n,3), got {tuple(x.shape)} / {tuple(wr.shape)}")
        C, H, W = x.shape
        out = torch.empty_like(x)
        check(_lib.lib().d3ga_blur_mix_fwd(C, H, W, wr.shape[0], dptr(x), dptr(wr), dptr(cell), dptr(out), stream_handle()),
              "d3ga_blur_mix_fwd")
        ctx.save_for_backward(x, wr, cell)
        return out

    @staticmethod
    def backward(ctx, g):
        x, wr, cell = ctx.saved_tensors
        C, H, W = x.shape
        g = f32c16(g)
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gw = part = None
        if ctx.needs_input_grad[1]:
            gw = torch.empty_like(wr)                      # written whole by the finishing stage: the camera's row, zeros elsewhere
            part = torch.empty(_lib.BLUR_PARTIALS, dtype=torch.float32, device=x.device)
        if gx is None and gw is None:
            return None, None, None
        check(_lib.lib().d3ga_blur_mix_bwd(C, H, W, wr.shape[0], dptr(x), dptr(wr), dptr(cell), dptr(g), dptr(gx), dptr(gw),
                                           dptr(part), stream_handle()), "d3ga_blur_mix_bwd")
        return gx, gw, None


def learnable_blur(img, weights_raw, cam_idx):
    """softmax(weights_raw[cam_idx]) mix of `img` (C,H,W), its 3x3 and its 7x7 Gaussian blur (reflect padding);
    models/learnable_blur.py:34-44 for one image.  Differentiable in img and weights_raw (n_cameras,3).  cam_idx: an int, or a
    (1,) int32 device tensor that the kernels read when they run -- put it in `CapturedStep(slots=...)` and a replay follows
    `replay(name=index)` without a new capture."""
    return _BlurMix.apply(img, weights_raw, _cam_cell(cam_idx, weights_raw.shape[0], img.device))


class LearnableBlur(nn.Module):
    """models/learnable_blur.py: same constructor, parameter (`weights_raw`, ones) and methods; reference checkpoints load
    with strict=True."""

    def __init__(self, cameras):
        super().__init__()
        self.cameras = copy.deepcopy(cameras)
        self.register_parameter("weights_raw", nn.Parameter(torch.ones(len(cameras), 3, dtype=torch.float32)))

    def name_to_idx(self, cameras):
        if isinstance(cameras, str):
            cameras = [cameras]
        return torch.tensor([self.cameras.index(c) for c in cameras], device=self.weights_raw.device, dtype=torch.long)

    def reg(self, cameras):
        return self.weights_raw[self.name_to_idx(cameras)]

    def forward(self, img, cameras):
        """img (B,C,H,W), one camera name per image (a single name for B = 1).  One launch per image; a camera that occurs
        twice in the batch receives the sum of both gradients (autograd adds the two whole-tensor gradients)."""
        if isinstance(cameras, str):
            cameras = [cameras]
        if img.dim() != 4 or img.shape[0] != len(cameras):
            raise ValueError(f"LearnableBlur: expected img (B,C,H,W) with one camera per image, got {tuple(img.shape)} and {len(cameras)} cameras")
        outs = [learnable_blur(img[b], self.weights_raw, self.cameras.index(c)) for b, c in enumerate(cameras)]
        return outs[0][None] if len(outs) == 1 else torch.stack(outs)


def compose_target(image, alpha, silhouette, boundary_fg, bg_color):
    """train.py:182-188 in one launch: with m = 1 - boundary_fg.float(),
        gt_image = (image * alpha + (1 - alpha) * bg) * m + (1 - m) * bg,     gt_silhouette = silhouette * alpha * m.
    image (C,H,W); alpha (1,H,W); silhouette (C,H,W) or (1,H,W); boundary_fg (1,H,W) bool, uint8 or float; bg_color (C) on
    the GPU (the random background of models/trainer.py:96-100).  No gradient.  Returns (gt_image, gt_silhouette)."""
    require_cuda(image, alpha, silhouette, boundary_fg, bg_color)
    with torch.no_grad():
        img = f32c16(image)
        if img.dim() != 3:
            raise ValueError(f"compose_target: expected image (C,H,W), got {tuple(img.shape)}")
        C, H, W = img.shape
        a = f32c16(alpha).reshape(-1)
        sil = f32c16(silhouette.expand(C, H, W))
        b = boundary_fg
        if b.dtype == torch.bool:
            b = b.contiguous().view(torch.uint8)
        elif b.dtype != torch.uint8:
            b = b.float()
        b = b.contiguous().reshape(-1)
        bg = f32c16(bg_color).reshape(-1)
        if a.numel() != H * W or b.numel() != H * W or bg.numel() != C:
            raise ValueError(f"compose_target: alpha / boundary_fg must hold H*W = {H * W} values and bg_color {C}, got "
                             f"{a.numel()} / {b.numel()} / {bg.numel()}")
        gt, gt_sil = torch.empty_like(img), torch.empty_like(img)
        check(_lib.lib().d3ga_compose_target(C, H, W, dptr(img), dptr(a), dptr(sil), dptr(b), int(b.dtype != torch.uint8),
                                             dptr(bg), dptr(gt), dptr(gt_sil), stream_handle()), "d3ga_compose_target")
    return gt, gt_sil
