"""Per-camera colour calibration and pixel bias of the Goliath configuration (configs/goliath_axe184.yml: use_color_calib,
use_pixel_cal).

Drop-ins for the reference's
    lib/calibration.py      CameraCalibration   (models/garment_net.py:12,44,265-266)
    models/color_calib.py   CameraPixelBias     (models/garment_net.py:17,46; models/trainer.py:128-131)
each one HIP launch per direction plus a one-workgroup finishing launch behind the colour backward (csrc/calib.hip).  GPU
tensors only; every op runs inside graph.CapturedStep with the camera index in `slots=`.
"""
import torch
from torch import nn

from . import _lib
from ._lib import check, dptr, f32c16, require_cuda, stream_handle

_cam_cells = {}


def _cam_cells_for(cam_idx, k, n_cameras, device, what):
    """cam_idx as the (k,) int32 device tensor the kernels read.  Host integers are validated here and served from a small
    per-device table (no host-to-device copy per call); a device tensor is the caller's -- the kernels clamp it."""
    if torch.is_tensor(cam_idx) and cam_idx.is_cuda:
        if cam_idx.dtype != torch.int32 or cam_idx.numel() != k:
            raise ValueError(f"{what}: cam_idx must be an int, {k} ints or a ({k},) int32 tensor on the GPU")
        require_cuda(cam_idx)
        return cam_idx.contiguous()
    if torch.is_tensor(cam_idx):
        cam_idx = cam_idx.tolist()
    idx = tuple(int(i) for i in cam_idx) if isinstance(cam_idx, (list, tuple)) else (int(cam_idx),)
    if len(idx) != k:
        raise ValueError(f"{what}: {len(idx)} camera indices for {k} views")
    for i in idx:
        if not 0 <= i < n_cameras:
            raise IndexError(f"{what}: camera index {i} outside [0, {n_cameras})")
    key = (device.index, idx)
    if key not in _cam_cells:
        if len(_cam_cells) >= 4096:                          # (160 cameras x a few batch shapes stays far below)
            _cam_cells.clear()
        _cam_cells[key] = torch.tensor(idx, dtype=torch.int32, device=device)
    return _cam_cells[key]


class _ColorCalib(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rgb, corrections, cells, identity_idx, grad_scale, planar):
        require_cuda(rgb, corrections)
        x = f32c16(rgb)
        cor = f32c16(corrections)
        k, n = (x.shape[0], x.shape[2]) if planar else (x.shape[0], x.shape[1])
        out = torch.empty_like(x)
        check(_lib.lib().d3ga_color_calib_fwd(k, n, int(planar), cor.shape[0], identity_idx, dptr(x), dptr(cor), dptr(cells),
                                              dptr(out), stream_handle()), "d3ga_color_calib_fwd")
        ctx.save_for_backward(x, cor, cells)
        ctx.args = (k, n, int(planar), identity_idx, float(grad_scale))
        return out

    @staticmethod
    def backward(ctx, g):
        x, cor, cells = ctx.saved_tensors
        k, n, planar, identity_idx, grad_scale = ctx.args
        gx = gc = part = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
        if ctx.needs_input_grad[1]:
            gc = torch.empty_like(cor)                       # written whole by the finishing stage
            part = torch.empty(_lib.CALIB_PARTIALS, dtype=torch.float32, device=x.device)
        if gx is None and gc is None:
            return None, None, None, None, None, None
        g = f32c16(g)
        check(_lib.lib().d3ga_color_calib_bwd(k, n, planar, cor.shape[0], identity_idx, grad_scale, dptr(x), dptr(cor), dptr(cells),
                                              dptr(g), dptr(gx), dptr(gc), dptr(part), stream_handle()), "d3ga_color_calib_bwd")
        return gx, gc, None, None, None, None


def color_calib(rgb, corrections, cam_idx, identity_idx, *, grad_scale=1.0, channels_first=False):
    """out = rgb * w + b per channel with (w, b) = corrections[cam][:3], corrections[cam][3:] (lib/calibration.py:45-50),
    bit-equal to that float32 expression; the views of camera `identity_idx` (None or negative: no such camera) are copied
    through unchanged.  rgb: (P,3) or (k,P,3); with channels_first=True (3,H,W) or (k,3,H,W).  corrections (n_cameras,6).
    cam_idx: an int, a sequence of k ints, or a (k,) int32 device tensor that the kernels read when they run -- put it in
    `CapturedStep(slots=...)` and a replay follows `replay(name=indices)` without a new capture.
    Differentiable in rgb and corrections.  dL/dcorrections is the whole tensor, multiplied by `grad_scale` (the reference's
    `params.register_hook(... 1e-1)` in training mode; dL/drgb is not scaled): exact zeros in the rows of cameras that are not
    in the batch AND in the identity camera's row.  The reference, asked for the identity camera by name, returns its input
    and the parameter receives NO gradient (None: Adam's momentum then leaves it alone, where a zero gradient would still
    move it); an op whose index lives on the device cannot decide that on the host, so this form yields the zero row.
    `CameraCalibration.forward` below keeps the reference's behaviour for a camera given by name."""
    x = rgb
    if x.dim() not in (2, 3) and not channels_first or channels_first and x.dim() not in (3, 4):
        raise ValueError(f"color_calib: expected rgb (P,3) / (k,P,3), or (3,H,W) / (k,3,H,W) with channels_first, got {tuple(x.shape)}")
    single = x.dim() == (3 if channels_first else 2)
    if single:
        x = x[None]
    if x.shape[1 if channels_first else 2] != 3:
        raise ValueError(f"color_calib: expected three channels, got {tuple(rgb.shape)} (channels_first={channels_first})")
    if corrections.dim() != 2 or corrections.shape[1] != 6:
        raise ValueError(f"color_calib: expected corrections (n_cameras,6), got {tuple(corrections.shape)}")
    require_cuda(x, corrections)
    ident = -1 if identity_idx is None else int(identity_idx)
    if ident >= corrections.shape[0]:
        raise IndexError(f"color_calib: identity_idx {ident} outside [0, {corrections.shape[0]})")
    cells = _cam_cells_for(cam_idx, x.shape[0], corrections.shape[0], x.device, "color_calib")
    shape = x.shape
    if channels_first:
        x = x.reshape(shape[0], 3, shape[2] * shape[3])
    out = _ColorCalib.apply(x, corrections, cells, max(ident, -1), grad_scale, channels_first).reshape(shape)
    return out[0] if single else out


class _PixelBias(torch.autograd.Function):
    @staticmethod
    def forward(ctx, bias, image, cell, H, W):
        require_cuda(bias, image)
        b = bias.float().contiguous()
        n, _, bh, bw = b.shape
        if image is None:
            C, img = 1, None
            out = torch.empty(1, H, W, dtype=torch.float32, device=b.device)
        else:
            img = image.float().contiguous()
            C = img.shape[0]
            out = torch.empty_like(img)
        check(_lib.lib().d3ga_pixel_bias_fwd(C, H, W, n, bh, bw, dptr(b), dptr(cell), dptr(img), dptr(out), stream_handle()),
              "d3ga_pixel_bias_fwd")
        ctx.save_for_backward(cell)
        ctx.args = (C, H, W, tuple(b.shape))
        return out

    @staticmethod
    def backward(ctx, g):
        (cell,) = ctx.saved_tensors
        C, H, W, shape = ctx.args
        gb = None
        if ctx.needs_input_grad[0]:
            g = g.float().contiguous()
            gb = torch.empty(shape, dtype=torch.float32, device=g.device)     # written whole: the camera's map, zeros elsewhere
            check(_lib.lib().d3ga_pixel_bias_bwd(C, H, W, shape[0], shape[2], shape[3], dptr(cell), dptr(g), dptr(gb), stream_handle()),
                  "d3ga_pixel_bias_bwd")
        return gb, (g if ctx.needs_input_grad[1] else None), None, None, None


def _check_bias(bias, what):
    if bias.dim() != 4 or bias.shape[1] != 1:
        raise ValueError(f"{what}: expected bias (n_cameras,1,h,w), got {tuple(bias.shape)}")


def pixel_bias(bias, cam_idx, height, width):
    """F.interpolate(bias[cam_idx][None], size=(height, width), mode='bilinear')[0] -> (1,H,W) (models/color_calib.py:257 for one
    index).  bias (n_cameras,1,h,w); cam_idx: an int or a (1,) int32 device tensor (see color_calib).  Differentiable in bias:
    the whole tensor's gradient is written, the camera's map by a gather over the pixels that touch each cell, zeros elsewhere."""
    _check_bias(bias, "pixel_bias")
    require_cuda(bias)
    cell = _cam_cells_for(cam_idx, 1, bias.shape[0], bias.device, "pixel_bias")
    return _PixelBias.apply(bias, None, cell, int(height), int(width))


def pixel_bias_add(image, bias, cam_idx):
    """image (C,H,W) + pixel_bias(bias, cam_idx, H, W), the sum of models/trainer.py:128-131, in the launch that upsamples
    (one read of the image); bit-equal to the two-step form.  Differentiable in image (the upstream gradient itself) and bias."""
    _check_bias(bias, "pixel_bias_add")
    if image.dim() != 3:
        raise ValueError(f"pixel_bias_add: expected image (C,H,W), got {tuple(image.shape)}")
    require_cuda(image, bias)
    cell = _cam_cells_for(cam_idx, 1, bias.shape[0], bias.device, "pixel_bias_add")
    return _PixelBias.apply(bias, image, cell, int(image.shape[1]), int(image.shape[2]))


class CameraCalibration(nn.Module):
    """lib/calibration.py: same constructor, attributes, parameter (`corrections`, every row [1,1,1,0,0,0]) and dispatch;
    reference checkpoints (`learnable_calib.*`) load with strict=True.  Created on the CPU; follows .cuda() / .to()."""

    def __init__(self, cameras, identity_camera=None):
        super().__init__()
        if identity_camera is None or identity_camera not in cameras:
            identity_camera = cameras[0]
        self.n_cameras = len(cameras)
        self.identity_camera = identity_camera
        self.cameras = cameras
        self.identity_idx = cameras.index(identity_camera)
        self.corrections = nn.Parameter(torch.tensor([[1., 1., 1., 0., 0., 0.]]).repeat(self.n_cameras, 1))
        self.cam2index = {cam: i for i, cam in enumerate(cameras)}

    def forward(self, rbg, cam_name):
        """A 3-D input is a (3,H,W) image, anything else is (...,3).  For the identity camera the INPUT TENSOR ITSELF is
        returned (lib/calibration.py:42-43) and `corrections` receives no gradient at all.  In training mode the parameter's
        gradient is scaled by 0.1 (the reference's register_hook, lines 52-54)."""
        idx = self.cam2index[cam_name]
        if self.identity_camera == cam_name:
            return rbg
        scale = 1e-1 if self.training and self.corrections.requires_grad else 1.0
        if rbg.dim() == 3:
            return color_calib(rbg, self.corrections, idx, self.identity_idx, grad_scale=scale, channels_first=True)
        return color_calib(rbg.reshape(rbg.numel() // 3, 3), self.corrections, idx, self.identity_idx, grad_scale=scale).reshape(rbg.shape)


class CameraPixelBias(nn.Module):
    """models/color_calib.py:245-258: same constructor and parameter (`bias`, zeros, (n_cameras,1,image_width // ds_rate,
    image_height // ds_rate) -- the reference's swap of the two sizes, kept so that its checkpoints load)."""

    def __init__(self, image_height, image_width, ds_rate, cameras):
        super().__init__()
        self.image_height = image_height
        self.image_width = image_width
        self.cameras = cameras
        self.n_cameras = len(cameras)
        bias = torch.zeros((self.n_cameras, 1, image_width // ds_rate, image_height // ds_rate), dtype=torch.float32)
        self.register_parameter("bias", nn.Parameter(bias))

    def forward(self, idxs):
        """idxs: an int, a sequence or a tensor of B camera indices -> (B,1,H,W); one launch per index (a (1,) int32 device
        tensor is read by the kernel, anything else on the host)."""
        if torch.is_tensor(idxs) and idxs.is_cuda and idxs.dtype == torch.int32 and idxs.numel() == 1:
            return pixel_bias(self.bias, idxs.reshape(1), self.image_height, self.image_width)[None]
        if torch.is_tensor(idxs):
            idxs = idxs.reshape(-1).tolist()
        elif not isinstance(idxs, (list, tuple)):
            idxs = [idxs]
        outs = [pixel_bias(self.bias, int(i), self.image_height, self.image_width) for i in idxs]
        return outs[0][None] if len(outs) == 1 else torch.stack(outs)
