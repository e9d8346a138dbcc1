"""VGG19 perceptual loss: drop-in for the reference's `VGGLoss` (utils/loss_utils.py:109-160; train.py:91, 212-214).

    loss = sum over taps relu1_1, relu2_1, relu3_1, relu4_1, relu5_1 (the first `n_layers`) of mean |f(pred) - f(gt)|

on images in [0, 1] as they are (no x255, no ImageNet normalisation), after the reference's `downsize` (the 2x2 box mean of
x[:2 floor(H/2), :2 floor(W/2)] -- exactly what F.interpolate(scale_factor=0.5, mode="bilinear") computes -- except for an
image of exactly 512 x 512, which passes unchanged).  Every step is a HIP launch of csrc/perceptual.hip on the current
stream: no torchvision, no MIOpen workspace, no host read-back, so the loss runs inside `torch.cuda.graph`.  GPU only.

Departure from the reference, kept on purpose: its `random_crop` slices `min(i, 0) : max(i + size, h)`, which is the whole
image, so nothing is ever cropped -- but when a side of the downsized image exceeds 512 it still consumes two host
`torch.randint` draws.  This module crops nothing either and draws NO random numbers (`plan(...).rng_draws` reports the two
draws the reference would have made), so the host RNG stream of a training run differs from the reference's after step
`enable_vgg_from` for such image sizes.

The weights are frozen: `gt` receives no gradient, and only dL/dpred is computed (the input gradient of a 3x3 convolution is
the same kernel over dY (.) [Y > 0] with flipped, transposed weight panels, packed once per weight set).
"""
import collections
import ctypes

import torch
from torch import nn

from . import _lib
from ._lib import check, dptr, require_cuda, stream_handle

CONV_KEYS = (0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28)      # torchvision's vgg19().features indices of conv1_1 .. conv5_1
POOL_BEFORE = (2, 4, 8, 12)                                       # conv indices with a 2x2 max pool in front
TAPS = (0, 2, 4, 8, 12)                                           # conv indices whose ReLU output is a feature tap
VGG19_WIDTHS = (64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512, 512)

Plan = collections.namedtuple("Plan", "down image convs taps rng_draws")


def n_convs(n_layers):
    if not 1 <= int(n_layers) <= 5:
        raise ValueError(f"VGGLoss: n_layers must be 1..5, got {n_layers}")
    return TAPS[int(n_layers) - 1] + 1


def plan(H, W, n_layers=5, downsize=True):
    """Host only.  The size at every level for an (H, W) image:
    down       whether `downsize` halves the image (False for exactly 512 x 512, and with downsize=False)
    image      (h, w) the chain sees -- what the reference's downsize + random_crop return (the crop never crops)
    convs      (h, w) of every convolution's output, conv1_1 first
    taps       (h, w) of the `n_layers` feature taps
    rng_draws  host randint draws the reference consumes for this size (2 when a side of `image` exceeds 512); none here"""
    H, W = int(H), int(W)
    nc = n_convs(n_layers)
    down = bool(downsize) and not (H == 512 and W == 512)
    h, w = (H // 2, W // 2) if down else (H, W)
    if H < 1 or W < 1 or h < 1 or w < 1:
        raise ValueError(f"VGGLoss: image {H} x {W} is too small")
    image = (h, w)
    convs = []
    for i in range(nc):
        if i in POOL_BEFORE:
            h, w = h // 2, w // 2
            if h < 1 or w < 1:
                raise ValueError(f"VGGLoss: image {H} x {W} is too small for the pool in front of conv index {i}")
        convs.append((h, w))
    return Plan(down, image, tuple(convs), tuple(convs[t] for t in TAPS[:n_layers]), 0 if max(image) <= 512 else 2)


def read_state_dict(weights, what="VGGLoss"):
    """A state dict as it is, or the one a path names (loaded with weights_only=True)."""
    if isinstance(weights, (str, bytes)) or hasattr(weights, "__fspath__"):
        weights = torch.load(weights, map_location="cpu", weights_only=True)
    if not hasattr(weights, "keys"):
        raise TypeError(f"{what}: weights must be a state dict or a path to one")
    return weights


def state_tensor(weights, names, what="VGGLoss"):
    """(the first of `names` the dict has, its tensor as float32); KeyError naming every candidate."""
    found = [n for n in names if n in weights]
    if not found:
        raise KeyError(f"{what}: the state dict has " + ("neither " + " nor ".join(repr(n) for n in names) if len(names) > 1
                                                           else f"no {names[0]!r}"))
    t = weights[found[0]]
    if not torch.is_tensor(t) or not t.is_floating_point():
        raise ValueError(f"{what}: {found[0]} is not a floating-point tensor")
    return found[0], t.detach().to(torch.float32)


def load_conv_chain(weights, conv_keys, prefixes=("features.{k}", "{k}"), what="VGGLoss"):
    """[(weight (Cout,Cin,3,3), bias (Cout))] float32 of the 3x3 convolutions `conv_keys` of a state dict (or a path to one), key
    K found as `<prefix>.weight` / `<prefix>.bias` under the first of `prefixes` (formatted with k=K, or a function K -> list of
    prefixes) the dict has.  Any widths are accepted as long as they chain: Cin of the first is 3, of every other the Cout before."""
    weights = read_state_dict(weights, what)
    out, cin = [], 3
    for k in conv_keys:
        pre = prefixes(k) if callable(prefixes) else [p.format(k=k) for p in prefixes]
        (wn, w), (bn, b) = (state_tensor(weights, [f"{p}.{leaf}" for p in pre], what) for leaf in ("weight", "bias"))
        if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or w.shape[1] != cin or w.shape[0] < 1:
            raise ValueError(f"{what}: {wn} must be (Cout, {cin}, 3, 3), got {tuple(w.shape)}")
        if tuple(b.shape) != (w.shape[0],):
            raise ValueError(f"{what}: {bn} must be ({w.shape[0]},), got {tuple(b.shape)}")
        out.append((w.contiguous(), b.contiguous()))
        cin = w.shape[0]
    return out


def load_vgg_weights(weights, n_layers=5):
    """[(weight (Cout,Cin,3,3), bias (Cout))] float32 for the convolutions `n_layers` needs, from a torchvision-style state dict
    (keys `features.K.weight` / `features.K.bias` or `K.weight` / `K.bias`, K in CONV_KEYS) or a path to one (loaded with
    weights_only=True).  Any widths are accepted as long as they chain: Cin of the first is 3, of every other the Cout before."""
    return load_conv_chain(weights, CONV_KEYS[:n_convs(n_layers)])


def _torchvision_weights():
    try:
        from torchvision import models
    except ImportError as e:
        raise ImportError("VGGLoss(weights=None) takes torchvision's default VGG19 weights, and torchvision is not installed: "
                          "pass weights= a state dict of vgg19 (or a path to one) instead") from e
    return models.vgg19(weights=models.VGG19_Weights.DEFAULT).features.state_dict()


# ---- thin wrappers over the single operations (channels-last float32 activations) -----------------------------------

def _act(x, what):
    require_cuda(x)
    if x.dtype != torch.float32 or x.dim() != 3 or not x.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous float32 (H, W, C) tensor, got {x.dtype} {tuple(x.shape)}")
    return x


def _out(out, shape, like, what):
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=like.device)
    if out.dtype != torch.float32 or tuple(out.shape) != tuple(shape) or not out.is_contiguous() or out.device != like.device:
        raise ValueError(f"{what}: out must be a contiguous float32 {tuple(shape)} tensor on {like.device}")
    return out


def pack_conv_weights(weight):
    """weight (Cout, Cin, 3, 3) on the GPU -> (forward panel, input-gradient panel), uint8 tensors; once per weight set."""
    require_cuda(weight)
    w = weight.detach().to(torch.float32).contiguous()
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3):
        raise ValueError(f"pack_conv_weights: expected (Cout, Cin, 3, 3), got {tuple(w.shape)}")
    cout, cin = w.shape[0], w.shape[1]
    L = _lib.lib()
    panels = []
    for transposed, (gi, go) in enumerate(((cin, cout), (cout, cin))):
        nbytes = L.d3ga_vgg_panel_bytes(gi, go)
        if nbytes < 0:
            check(int(nbytes), "d3ga_vgg_panel_bytes")
        p = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
        check(L.d3ga_vgg_pack_weights(cout, cin, dptr(w), transposed, dptr(p), stream_handle()), "d3ga_vgg_pack_weights")
        panels.append(p)
    return panels[0], panels[1]


def conv3x3_relu(x, panel, bias, cout, relu=True, out=None):
    """y (H, W, cout) = relu(conv3x3(x, pad 1) + bias) for x (H, W, Cin) and the forward panel of pack_conv_weights."""
    x = _act(x, "conv3x3_relu")
    H, W, cin = x.shape
    y = _out(out, (H, W, cout), x, "conv3x3_relu")
    check(_lib.lib().d3ga_vgg_conv3x3(H, W, cin, cout, dptr(x), None, dptr(panel), dptr(bias), int(bool(relu)), 0, dptr(y),
                                      stream_handle()), "d3ga_vgg_conv3x3")
    return y


def conv3x3_relu_bwd(gy, y, panel_t, cin, out=None, accumulate=False):
    """dL/dx (H, W, cin) of y = relu(conv3x3(x) + bias) from gy and the stored activation y (the mask is y > 0), with the
    input-gradient panel of pack_conv_weights.  accumulate: add to `out` instead of overwriting it."""
    gy, y = _act(gy, "conv3x3_relu_bwd"), _act(y, "conv3x3_relu_bwd")
    if gy.shape != y.shape:
        raise ValueError(f"conv3x3_relu_bwd: gy {tuple(gy.shape)} and y {tuple(y.shape)} differ")
    if accumulate and out is None:
        raise ValueError("conv3x3_relu_bwd: accumulate needs out")
    H, W, cout = y.shape
    gx = _out(out, (H, W, cin), y, "conv3x3_relu_bwd")
    check(_lib.lib().d3ga_vgg_conv3x3(H, W, cout, cin, dptr(gy), dptr(y), dptr(panel_t), None, 0, int(bool(accumulate)), dptr(gx),
                                      stream_handle()), "d3ga_vgg_conv3x3")
    return gx


def maxpool2(x, out=None):
    x = _act(x, "maxpool2")
    H, W, C = x.shape
    y = _out(out, (H // 2, W // 2, C), x, "maxpool2")
    check(_lib.lib().d3ga_vgg_maxpool2_fwd(H, W, C, dptr(x), dptr(y), stream_handle()), "d3ga_vgg_maxpool2_fwd")
    return y


def _act_n(x, what):
    require_cuda(x)
    if x.dtype != torch.float32 or x.dim() != 4 or not x.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous float32 (N, H, W, C) tensor, got {x.dtype} {tuple(x.shape)}")
    return x


def conv3x3_n(x, panel, bias, cout, relu=True, out=None, mask_y=None, accumulate=False):
    """The convolution over N images at once (d3ga_vgg_conv3x3_n): x (N, H, W, Cin) -> y (N, H, W, cout), the images sharing
    every weight load; image n is bit for bit conv3x3_relu / conv3x3_relu_bwd on x[n].  mask_y (N, H, W, Cin): x is zeroed
    where mask_y <= 0 (the input-gradient form, with the transposed panel and bias None); accumulate: add to `out`."""
    x = _act_n(x, "conv3x3_n")
    N, H, W, cin = x.shape
    if mask_y is not None and _act_n(mask_y, "conv3x3_n").shape != x.shape:
        raise ValueError(f"conv3x3_n: mask_y {tuple(mask_y.shape)} and x {tuple(x.shape)} differ")
    if accumulate and out is None:
        raise ValueError("conv3x3_n: accumulate needs out")
    y = _out(out, (N, H, W, cout), x, "conv3x3_n")
    check(_lib.lib().d3ga_vgg_conv3x3_n(N, H, W, cin, cout, dptr(x), dptr(mask_y), dptr(panel), dptr(bias), int(bool(relu)),
                                        int(bool(accumulate)), dptr(y), stream_handle()), "d3ga_vgg_conv3x3_n")
    return y


def maxpool2_n(x, out=None):
    """maxpool2 over N images at once: x (N, H, W, C) -> (N, H/2, W/2, C)."""
    x = _act_n(x, "maxpool2_n")
    N, H, W, C = x.shape
    y = _out(out, (N, H // 2, W // 2, C), x, "maxpool2_n")
    check(_lib.lib().d3ga_vgg_maxpool2_fwd_n(N, H, W, C, dptr(x), dptr(y), stream_handle()), "d3ga_vgg_maxpool2_fwd_n")
    return y


def maxpool2_bwd(x, gy, out=None):
    """dL/dx of y = maxpool2(x): the first maximum of a window (row-major) takes the gradient; a dropped row / column zeros."""
    x, gy = _act(x, "maxpool2_bwd"), _act(gy, "maxpool2_bwd")
    H, W, C = x.shape
    if tuple(gy.shape) != (H // 2, W // 2, C):
        raise ValueError(f"maxpool2_bwd: gy must be {(H // 2, W // 2, C)}, got {tuple(gy.shape)}")
    gx = _out(out, (H, W, C), x, "maxpool2_bwd")
    check(_lib.lib().d3ga_vgg_maxpool2_bwd(H, W, C, dptr(x), dptr(gy), dptr(gx), stream_handle()), "d3ga_vgg_maxpool2_bwd")
    return gx


def _img(img, what):
    require_cuda(img)
    if img.dtype != torch.float32 or img.dim() != 3:
        raise ValueError(f"{what}: expected a float32 (C, H, W) image, got {img.dtype} {tuple(img.shape)}")
    return img.contiguous()


def box_down2(img, down=True, out=None):
    """img (C, H, W) -> channels-last (H/2, W/2, C): the reference's `downsize`; down=False: the transpose alone."""
    img = _img(img, "box_down2")
    C, H, W = img.shape
    y = _out(out, (H // 2, W // 2, C) if down else (H, W, C), img, "box_down2")
    check(_lib.lib().d3ga_vgg_box_down2_fwd(C, H, W, int(bool(down)), dptr(img), dptr(y), stream_handle()), "d3ga_vgg_box_down2_fwd")
    return y


def box_down2_bwd(g, H, W, down=True):
    """dL/dimg (C, H, W) from g, the gradient of box_down2's output."""
    g = _act(g, "box_down2_bwd")
    C = g.shape[2]
    if tuple(g.shape[:2]) != ((H // 2, W // 2) if down else (H, W)):
        raise ValueError(f"box_down2_bwd: g {tuple(g.shape)} does not belong to a {H} x {W} image")
    gi = torch.empty((C, H, W), dtype=torch.float32, device=g.device)
    check(_lib.lib().d3ga_vgg_box_down2_bwd(C, H, W, int(bool(down)), dptr(g), dptr(gi), stream_handle()), "d3ga_vgg_box_down2_bwd")
    return gi


def l1_mean(a, b, out, partials):
    """out[0] = mean |a - b| (two stages, reproducible bit for bit); partials: _lib.LOSS_PARTIALS floats of scratch."""
    check(_lib.lib().d3ga_l1_mean_fwd_ws(a.numel(), dptr(a), dptr(b), dptr(out), dptr(partials), stream_handle()), "d3ga_l1_mean_fwd_ws")
    return out


def l1_mean_grad(a, b, g, out=None):
    """g[0] * sign(a - b) / n, sign(0) = 0; g a (1,) device tensor."""
    ga = _out(out, a.shape, a, "l1_mean_grad")
    check(_lib.lib().d3ga_l1_mean_bwd(a.numel(), dptr(a), dptr(b), dptr(g), dptr(ga), stream_handle()), "d3ga_l1_mean_bwd")
    return ga


# ---- the chain ------------------------------------------------------------------------------------------------------

def _align256(n):
    return (n + 255) & ~255


def scratch_bytes(H, W, down, n_layers, widths):
    """d3ga_vgg_scratch_bytes: (saved-for-backward, forward work, backward work) bytes."""
    out = (ctypes.c_int64 * 3)()
    arr = (ctypes.c_int32 * 13)(*(list(widths) + [1] * (13 - len(widths))))
    check(_lib.lib().d3ga_vgg_scratch_bytes(int(H), int(W), int(bool(down)), int(n_layers), arr, out), "d3ga_vgg_scratch_bytes")
    return out[0], out[1], out[2]


class _Carver:
    """Consecutive float32 tensors, each on a 256-byte boundary, out of one caller-owned buffer."""

    def __init__(self, nbytes, device):
        self.buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        self.off = 0

    def take(self, *shape):
        n = 4
        for s in shape:
            n *= s
        if self.off + n > self.buf.numel():
            raise _lib.D3GAError("VGGLoss: the scratch layout and d3ga_vgg_scratch_bytes disagree")
        t = self.buf[self.off:self.off + n].view(torch.float32).view(*shape)
        self.off += _align256(n)
        return t


class _Chain:
    """What one forward of the source image leaves behind: the plan, every activation, the per-tap L1 gradients."""
    __slots__ = ("H", "W", "pl", "x0", "pooled", "acts", "tap_grads", "keep")


def _forward(mod, pred, gt, want_grad):
    """One image: loss (0-dim tensor), and the chain for the backward when want_grad."""
    C, H, W = pred.shape
    nc, widths = len(mod.widths), mod.widths
    pl = plan(H, W, mod.n_layers, mod.downsize)
    b_saved, b_work, _ = scratch_bytes(H, W, pl.down, mod.n_layers, widths)
    dev = pred.device
    saved, work = _Carver(b_saved, dev), _Carver(b_work, dev)
    biggest = max([3 * pl.image[0] * pl.image[1]] + [h * w * c for (h, w), c in zip(pl.convs, widths)])
    pp = [work.take(biggest), work.take(biggest)]
    partials, means = work.take(_lib.LOSS_PARTIALS), work.take(64)
    panels_f, biases, one = mod._panels_f, mod._biases, mod._one
    ch = _Chain()
    ch.H, ch.W, ch.pl, ch.pooled, ch.acts, ch.tap_grads, ch.keep = H, W, pl, {}, [], {}, saved
    ch.x0 = box_down2(pred, pl.down, out=saved.take(*pl.image, 3))
    t = box_down2(gt, pl.down, out=pp[0][:3 * pl.image[0] * pl.image[1]].view(*pl.image, 3))
    s, side, cin, tap = ch.x0, 1, 3, 0
    for i in range(nc):
        h, w = pl.convs[i]
        if i in POOL_BEFORE:
            s = maxpool2(s, out=saved.take(h, w, cin))
            ch.pooled[i] = s
            t = maxpool2(t, out=pp[side][:h * w * cin].view(h, w, cin))
            side ^= 1
        s = conv3x3_relu(s, panels_f[i], biases[i], widths[i], out=saved.take(h, w, widths[i]))
        t = conv3x3_relu(t, panels_f[i], biases[i], widths[i], out=pp[side][:h * w * widths[i]].view(h, w, widths[i]))
        side ^= 1
        ch.acts.append(s)
        if i in TAPS:
            l1_mean(s, t, means[tap:tap + 1], partials)
            if want_grad:
                ch.tap_grads[i] = l1_mean_grad(s, t, one, out=saved.take(h, w, widths[i]))
            tap += 1
        cin = widths[i]
    return means[:mod.n_layers].sum(), ch


def _backward(mod, ch):
    """dL/dpred (3, H, W) for an upstream gradient of one."""
    pl, widths = ch.pl, mod.widths
    nc = len(widths)
    _, _, b_bwd = scratch_bytes(ch.H, ch.W, pl.down, mod.n_layers, widths)
    work = _Carver(b_bwd, ch.x0.device)
    half = b_bwd // 8
    pp = [work.take(half), work.take(half)]
    g, side = ch.tap_grads[nc - 1], 0
    for i in range(nc - 1, -1, -1):
        h, w = pl.convs[i]
        cin = widths[i - 1] if i else 3
        dst = pp[side][:h * w * cin].view(h, w, cin)
        side ^= 1
        acc = (i - 1) in ch.tap_grads
        if acc:
            assert i not in POOL_BEFORE
            dst.copy_(ch.tap_grads[i - 1])
        g = conv3x3_relu_bwd(g, ch.acts[i], mod._panels_b[i], cin, out=dst, accumulate=acc)
        if i in POOL_BEFORE:
            x = ch.acts[i - 1]
            g = maxpool2_bwd(x, g, out=pp[side][:x.numel()].view(x.shape))
            side ^= 1
    return box_down2_bwd(g, ch.H, ch.W, pl.down)


class _VGGLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, mod):
        want = ctx.needs_input_grad[0]
        loss, ch = _forward(mod, pred, gt, want)
        ctx.mod, ctx.chain = mod, (ch if want else None)
        return loss

    @staticmethod
    def backward(ctx, g_out):
        if ctx.chain is None:
            return None, None, None
        return _backward(ctx.mod, ctx.chain) * g_out, None, None


class VGGLoss(nn.Module):
    """The reference's VGGLoss(n_layers) with the weights as an argument.

    weights: a torchvision-style vgg19 state dict or a path to one (see load_vgg_weights); None takes torchvision's default
    VGG19 weights as the reference does (lazy import; ImportError without torchvision).  The module holds buffers only (the
    raw weights, not persistent: the reference builds the loss outside the trainer and never checkpoints it); the packed
    weight panels are built on the first call on a device, or by `prepare()` -- call it (or run one step) before capturing."""

    def __init__(self, n_layers=5, weights=None, *, downsize=True):
        super().__init__()
        self.n_layers = int(n_layers)
        self.downsize = bool(downsize)      # False: the images are at working resolution already (not in the reference)
        n_convs(self.n_layers)
        pairs = load_vgg_weights(_torchvision_weights() if weights is None else weights, self.n_layers)
        self.widths = tuple(int(w.shape[0]) for w, _ in pairs)
        for i, (w, b) in enumerate(pairs):
            self.register_buffer(f"w{i}", w.clone(), persistent=False)
            self.register_buffer(f"b{i}", b.clone(), persistent=False)
        self.register_buffer("one", torch.ones(1, dtype=torch.float32), persistent=False)
        self._ready = None

    def prepare(self):
        """Pack the weight panels on the buffers' device (once per device / weight set)."""
        w0 = self.w0
        key = (w0.device, tuple(getattr(self, f"w{i}").data_ptr() for i in range(len(self.widths))))
        if self._ready != key:
            require_cuda(w0)
            packed = [pack_conv_weights(getattr(self, f"w{i}")) for i in range(len(self.widths))]
            self._panels_f = [p[0] for p in packed]
            self._panels_b = [p[1] for p in packed]
            self._biases = [getattr(self, f"b{i}") for i in range(len(self.widths))]
            self._one = self.one
            self._ready = key
        return self

    def _check(self, pred, gt):
        if pred.dim() == 3:
            pred, gt = pred[None], gt[None] if gt.dim() == 3 else gt
        if pred.dim() != 4 or pred.shape[1] != 3 or gt.shape != pred.shape:
            raise ValueError(f"VGGLoss: expected pred and gt of one shape (N,3,H,W) or (3,H,W), got {tuple(pred.shape)} / {tuple(gt.shape)}")
        require_cuda(pred, gt)
        return pred.float(), gt.detach().float()

    def forward(self, pred, gt):
        pred, gt = self._check(pred, gt)
        self.prepare()
        losses = [_VGGLossFn.apply(pred[n], gt[n], self) for n in range(pred.shape[0])]
        return losses[0] if len(losses) == 1 else torch.stack(losses).mean()

    def features(self, image):
        """The `n_layers` feature taps of one (3, H, W) image, channels-last (h, w, C) each (for tests and inspection)."""
        image, _ = self._check(image, image)
        self.prepare()
        with torch.no_grad():
            _, ch = _forward(self, image[0], image[0], False)
        return [ch.acts[t] for t in TAPS[:self.n_layers]]
