"""LPIPS (VGG): drop-in for `lpips.LPIPS("vgg")` of the reference's recorder/heatmap.py:13, 40 -- the third figure of
`errors_<trajectory>.txt` (test.py:171-174, 200-206) -- without the `lpips` package, torchvision or MIOpen.

    x'    = ((2 x - 1 if normalize else x) - shift) / scale              shift (-.030, -.088, -.188), scale (.458, .448, .450)
    f_t   = the ReLU outputs of VGG16 behind conv1_2, 2_2, 3_3, 4_3, 5_3 (13 convolutions, four 2x2 max pools, full resolution)
    d_t   = sum_c lin_t[c] (a_c / (|a| + 1e-10) - b_c / (|b| + 1e-10))^2   per pixel, a and b the two images' features
    value = sum_t mean over pixels of d_t

The reference feeds images in [0, 1] with normalize=False (the package expects [-1, 1]); that quirk is the default here.  Fake
and target run through every layer as ONE batch (csrc/perceptual.hip: d3ga_vgg_conv3x3_n), the head is csrc/lpips.hip.
Forward only -- a metric: the inputs are detached, nothing has a gradient.  Every step is a HIP launch on the current stream,
nothing is read back and no float atomics are used: image b of a batch is bit for bit the single-pair call, and a replay of
a captured call bit for bit the eager one.  GPU only.  One module serves one stream at a time (its work area is its own).

PARITY UNPINNED: the `lpips` package is not available where this was written.  The formula above, the layer positions and
the key names below are written from recall of the public package and the paper; tests hold the device against a plain
torch restatement (tests/lpips_ref.py) and against first-principles answers of the distance, not against the package.

Weights never come from anywhere but the caller: a state dict, a path to one (loaded with weights_only=True), or the path in
the environment variable D3GA_LPIPS_WEIGHTS.  Two key layouts are accepted (names from recall of the public packages):
  * torchvision's vgg16: `features.K.weight` / `features.K.bias`, K in CONV_KEYS, plus the linear heads
    `lin{0..4}.model.1.weight` of shape (1, C, 1, 1);
  * the package's own `LPIPS("vgg").state_dict()`: `net.slice{1..5}.K.weight` / `.bias`, with `lin{k}.model.1.weight` or
    `lins.k.model.1.weight`.
Any widths are accepted as long as they chain and every head matches its tap (a tap at most 512 wide).
"""
import collections
import ctypes
import os

import torch
from torch import nn

from . import _lib
from ._lib import check, dptr, require_cuda, stream_handle
from .perceptual import _Carver, conv3x3_n, load_conv_chain, maxpool2_n, pack_conv_weights, read_state_dict, state_tensor

CONV_KEYS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)      # torchvision's vgg16().features indices of conv1_1 .. conv5_3
POOL_BEFORE = (2, 4, 7, 10)                                       # conv indices with a 2x2 max pool in front
TAPS = (1, 3, 6, 9, 12)                                           # conv indices whose ReLU output is a feature tap
VGG16_WIDTHS = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
SHIFT, SCALE = (-.030, -.088, -.188), (.458, .448, .450)
MIN_SIDE = 16                                                     # four floor pools
MAX_TAP_WIDTH = 512
WEIGHTS_ENV = "D3GA_LPIPS_WEIGHTS"

Plan = collections.namedtuple("Plan", "convs taps")


def plan(H, W):
    """Host only.  (h, w) of every convolution's output and of the five taps for an (H, W) image; a side below 16 leaves
    nothing for the last tap: ValueError."""
    H, W = int(H), int(W)
    if H < MIN_SIDE or W < MIN_SIDE:
        raise ValueError(f"LPIPS: image {H} x {W} is too small: four 2x2 pools need sides of at least {MIN_SIDE}")
    h, w, convs = H, W, []
    for i in range(len(CONV_KEYS)):
        if i in POOL_BEFORE:
            h, w = h // 2, w // 2
        convs.append((h, w))
    return Plan(tuple(convs), tuple(convs[t] for t in TAPS))


def _slice_prefixes(k):
    s = 1 + sum(k > last for last in (2, 7, 14, 21))              # the package cuts features into slice1..5 behind these convs
    return [f"features.{k}", f"net.slice{s}.{k}"]


def load_lpips_weights(weights):
    """([(weight, bias)] x 13, [lin (C,)] x 5) float32 from a state dict or a path, in either layout of the module docstring."""
    weights = read_state_dict(weights, "LPIPS")
    pairs = load_conv_chain(weights, CONV_KEYS, _slice_prefixes, "LPIPS")
    lins = []
    for t, i in enumerate(TAPS):
        c = pairs[i][0].shape[0]
        name, l = state_tensor(weights, [f"lin{t}.model.1.weight", f"lins.{t}.model.1.weight"], "LPIPS")
        if tuple(l.shape) != (1, c, 1, 1):
            raise ValueError(f"LPIPS: {name} must be (1, {c}, 1, 1) for a tap of {c} channels, got {tuple(l.shape)}")
        if c > MAX_TAP_WIDTH:
            raise ValueError(f"LPIPS: {name}: a tap of {c} channels is wider than {MAX_TAP_WIDTH}")
        lins.append(l.reshape(c).contiguous())
    return pairs, lins


def _env_weights():
    path = os.environ.get(WEIGHTS_ENV)
    if not path:
        raise ImportError(
            f"LPIPS(weights=None) reads the state dict at ${WEIGHTS_ENV}, which is not set, and never fetches weights: pass "
            "weights= a state dict (or a path to one) in torchvision's vgg16 layout (features.K.weight/bias plus "
            "lin{0..4}.model.1.weight) or in the lpips package's own LPIPS('vgg').state_dict() layout "
            "(net.slice{1..5}.K.weight/bias plus lin{k}.model.1.weight or lins.k.model.1.weight)")
    return path


# ---- thin wrappers over the single operations -----------------------------------------------------------------------

def scale_input(img, normalize=False, out=None):
    """img (N, 3, H, W) float32 -> channels-last (N, H, W, 3) through the scaling layer (d3ga_lpips_input)."""
    require_cuda(img, out)
    if img.dtype != torch.float32 or img.dim() != 4 or img.shape[1] != 3 or not img.is_contiguous():
        raise ValueError(f"scale_input: expected a contiguous float32 (N, 3, H, W) tensor, got {img.dtype} {tuple(img.shape)}")
    N, _, H, W = img.shape
    if out is None:
        out = torch.empty((N, H, W, 3), dtype=torch.float32, device=img.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (N, H, W, 3) or not out.is_contiguous():
        raise ValueError(f"scale_input: out must be a contiguous float32 {(N, H, W, 3)} tensor")
    check(_lib.lib().d3ga_lpips_input(N, H, W, int(bool(normalize)), dptr(img), dptr(out), stream_handle()), "d3ga_lpips_input")
    return out


def tap_distance(a, b, lin, want_map=True, value=None, accumulate=False, partials=None):
    """Features a, b (B, h, w, C) and weights lin (C,) -> (value (B,), map (B, h, w) | None): the per-pixel distance of the module
    docstring and its spatial mean per image, stored into `value` or (accumulate) added to it.  partials: B *
    _lib.LPIPS_PARTIALS floats of scratch (allocated when None)."""
    require_cuda(a, b, lin, value, partials)
    for t in (a, b):
        if t.dtype != torch.float32 or t.dim() != 4 or not t.is_contiguous():
            raise ValueError(f"tap_distance: expected contiguous float32 (B, h, w, C) features, got {t.dtype} {tuple(t.shape)}")
    if a.shape != b.shape:
        raise ValueError(f"tap_distance: a {tuple(a.shape)} and b {tuple(b.shape)} differ")
    B, h, w, C = a.shape
    if lin.dtype != torch.float32 or tuple(lin.shape) != (C,) or not lin.is_contiguous():
        raise ValueError(f"tap_distance: lin must be a contiguous float32 ({C},) tensor, got {lin.dtype} {tuple(lin.shape)}")
    if not 1 <= C <= MAX_TAP_WIDTH:
        raise ValueError(f"tap_distance: C must be 1..{MAX_TAP_WIDTH}, got {C}")
    if accumulate and value is None:
        raise ValueError("tap_distance: accumulate needs value")
    if value is None:
        value = torch.empty(B, dtype=torch.float32, device=a.device)
    elif value.dtype != torch.float32 or tuple(value.shape) != (B,) or not value.is_contiguous():
        raise ValueError(f"tap_distance: value must be a contiguous float32 ({B},) tensor")
    if partials is None:
        partials = torch.empty(B * _lib.LPIPS_PARTIALS, dtype=torch.float32, device=a.device)
    elif partials.dtype != torch.float32 or partials.numel() < B * _lib.LPIPS_PARTIALS or not partials.is_contiguous():
        raise ValueError(f"tap_distance: partials must hold {B * _lib.LPIPS_PARTIALS} float32")
    m = torch.empty((B, h, w), dtype=torch.float32, device=a.device) if want_map else None
    check(_lib.lib().d3ga_lpips_tap(B, h, w, C, dptr(a), dptr(b), dptr(lin), dptr(m), dptr(partials), dptr(value),
                                    int(bool(accumulate)), stream_handle()), "d3ga_lpips_tap")
    return value, m


def scratch_bytes(B, H, W, widths):
    """d3ga_lpips_scratch_bytes: (all, one ping-pong buffer, partials) bytes of the work area of B image pairs."""
    out = (ctypes.c_int64 * 3)()
    arr = (ctypes.c_int32 * len(CONV_KEYS))(*widths)
    st = _lib.lib().d3ga_lpips_scratch_bytes(int(B), int(H), int(W), arr, out)
    if st == -2:                                                   # D3GA_E_SIZE
        raise ValueError(f"LPIPS: {B} pairs of {H} x {W} images: a side below {MIN_SIDE}, or an activation past 2^31 - 1 elements")
    check(st, "d3ga_lpips_scratch_bytes")
    return out[0], out[1], out[2]


class LPIPS(nn.Module):
    """`lpips.LPIPS("vgg")` with the weights as an argument (see the module docstring for the accepted forms).

    forward(fake, target): (3, H, W) or (B, 3, H, W) float32 device tensors -> (1, 1, 1, 1) or (B, 1, 1, 1), as the package
    returns; so it drops into `Evaluator(lpips=...)` and `compute_errors(..., lpips=...)`.  maps(fake, target): the five
    per-tap distance maps.  The module holds buffers only (not persistent).  The packed weight panels and the work area are
    built on the first call for a device and an image size, or by `prepare(H, W, B)` -- call it (or run once) before capturing."""

    def __init__(self, net="vgg", weights=None, *, normalize=False):
        super().__init__()
        if net != "vgg":
            raise NotImplementedError(f"LPIPS: only net='vgg' is implemented, got {net!r}")
        self.normalize = bool(normalize)
        pairs, lins = load_lpips_weights(_env_weights() if weights is None else weights)
        self.widths = tuple(int(w.shape[0]) for w, _ in pairs)
        for i, (w, b) in enumerate(pairs):
            self.register_buffer(f"w{i}", w.clone(), persistent=False)
            self.register_buffer(f"b{i}", b.clone(), persistent=False)
        for t, l in enumerate(lins):
            self.register_buffer(f"lin{t}", l.clone(), persistent=False)
        self._ready = None
        self._work_key = None

    def prepare(self, H=None, W=None, B=1):
        """Pack the weight panels on the buffers' device (once per device / weight set) and, given a size, allocate the work
        area of B pairs of (3, H, W) images."""
        w0 = self.w0
        require_cuda(w0)
        key = (w0.device, tuple(getattr(self, f"w{i}").data_ptr() for i in range(len(self.widths))))
        if self._ready != key:
            self._panels = [pack_conv_weights(getattr(self, f"w{i}"))[0] for i in range(len(self.widths))]
            self._biases = [getattr(self, f"b{i}") for i in range(len(self.widths))]
            self._lins = [getattr(self, f"lin{t}") for t in range(len(TAPS))]
            self._ready, self._work_key = key, None
        if H is not None:
            wkey = (w0.device, int(B), int(H), int(W))
            if self._work_key != wkey:
                plan(H, W)
                total, one, part = scratch_bytes(B, H, W, self.widths)
                work = _Carver(total, w0.device)
                self._pp = [work.take(one // 4), work.take(one // 4)]
                self._partials = work.take(part // 4)
                self._work, self._work_key = work, wkey
        return self

    def _check(self, fake, target):
        for t in (fake, target):
            if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() not in (3, 4) or t.shape[-3] != 3:
                raise ValueError("LPIPS: expected float32 images (3,H,W) or (B,3,H,W), got "
                                 f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
        if fake.shape != target.shape:
            raise ValueError(f"LPIPS: fake {tuple(fake.shape)} and target {tuple(target.shape)} differ")
        plan(fake.shape[-2], fake.shape[-1])
        require_cuda(fake, target)
        batched = fake.dim() == 4
        f, t = fake.detach().contiguous(), target.detach().contiguous()
        return (f, t, True) if batched else (f[None], t[None], False)

    def _run(self, fake, target, want_maps):
        B, _, H, W = fake.shape
        self.prepare(H, W, B)
        pl, widths, n = plan(H, W), self.widths, 2 * B
        pp, value, maps = self._pp, torch.empty(B, dtype=torch.float32, device=fake.device), []
        cur = pp[0][:n * H * W * 3].view(n, H, W, 3)
        scale_input(fake, self.normalize, out=cur[:B])
        scale_input(target, self.normalize, out=cur[B:])
        side, cin, tap = 1, 3, 0
        for i, c in enumerate(widths):
            h, w = pl.convs[i]
            if i in POOL_BEFORE:
                cur = maxpool2_n(cur, out=pp[side][:n * h * w * cin].view(n, h, w, cin))
                side ^= 1
            cur = conv3x3_n(cur, self._panels[i], self._biases[i], c, out=pp[side][:n * h * w * c].view(n, h, w, c))
            side ^= 1
            if i in TAPS:                                          # consumed here, before the buffers rotate
                _, m = tap_distance(cur[:B], cur[B:], self._lins[tap], want_maps, value, tap > 0, self._partials)
                maps.append(m)
                tap += 1
            cin = c
        return value, maps

    @torch.no_grad()
    def forward(self, fake, target):
        fake, target, _ = self._check(fake, target)
        value, _ = self._run(fake, target, False)
        return value.view(-1, 1, 1, 1)

    @torch.no_grad()
    def maps(self, fake, target):
        """The five per-tap distance maps, (B, h, w) each for (B,3,H,W) images and (h, w) for (3,H,W); their spatial means
        add up to forward()."""
        fake, target, batched = self._check(fake, target)
        _, maps = self._run(fake, target, True)
        return maps if batched else [m[0] for m in maps]
