"""Oracle of the VGG perceptual loss (d3ga_amd/perceptual.py): the reference's VGGLoss.forward (utils/loss_utils.py:109-160)
restated as plain torch on the CPU, in any dtype (float64 is the yardstick, float32 gives e32, the float32 evaluation's own
error).  Also the single operations, seeded weights and inputs, and the seed qualification of the end-to-end gradient tests.
"""
import numpy as np
import torch
import torch.nn.functional as F

CONV_KEYS = (0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28)
POOL_BEFORE = (2, 4, 8, 12)
TAPS = (0, 2, 4, 8, 12)
VGG19_WIDTHS = (64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512, 512)
NARROW_WIDTHS = (8, 8, 16, 20, 24, 24, 40, 24, 40, 33, 40, 40, 48)
GOLDEN_WIDTHS = (8, 8, 12, 10, 16, 16, 20, 16, 24, 17, 24, 24, 24)      # of tests/golden/vgg_cases.npz (tools/gen_perceptual_golden.py)
# seeds of the narrow end-to-end cases, per image size: every one qualifies (see `qualify`); asserted by test_perceptual_host.py
NARROW_SEEDS = {(37, 53): (0, 2, 3, 5), (40, 56): (3, 4, 7, 8)}      # weights make_weights(NARROW_WIDTHS, s), images make_images(H, W, s)
NARROW_BATCH = ((37, 53), 0, (0, 1))      # N = 2: weights of seed 0, images of seeds 0 and 1
GOLDEN_SEED = 9                           # weights; images of seeds 9 (37x53) and 10 (40x56)
GOLDEN_BAR = (1e-3, 1e-6)          # the project's element-wise bar |a - b| <= 1e-3 |b| + 1e-6 max|b|


def make_weights(widths, seed, style="features"):
    """He-initialised seeded state dict (float32) in torchvision's key layout; biases uniform in +-0.1."""
    g = torch.Generator().manual_seed(1000 + seed)
    sd, cin = {}, 3
    for k, c in zip(CONV_KEYS, widths):
        pre = f"features.{k}" if style == "features" else f"{k}"
        sd[pre + ".weight"] = torch.randn(c, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
        sd[pre + ".bias"] = (torch.rand(c, generator=g) - 0.5) * 0.2
        cin = c
    return sd


def make_images(H, W, seed, n=None):
    """pred, gt in [0, 1], float32: gt = rand, pred = clamp(gt + 0.25 randn, 0, 1)."""
    g = torch.Generator().manual_seed(2000 + seed)
    shape = (3, H, W) if n is None else (n, 3, H, W)
    gt = torch.rand(shape, generator=g)
    return (gt + 0.25 * torch.randn(shape, generator=g)).clamp(0, 1), gt


def pairs_of(sd, n_convs):
    out = []
    for k in CONV_KEYS[:n_convs]:
        pre = f"features.{k}" if f"features.{k}.weight" in sd else f"{k}"
        out.append((torch.as_tensor(sd[pre + ".weight"]), torch.as_tensor(sd[pre + ".bias"])))
    return out


def downsize(x, enabled=True):
    """(3,H,W) -> the reference's downsize: unchanged at exactly 512 x 512, else the 2x2 box mean (an odd row / column dropped)."""
    if not enabled or (x.shape[-2] == 512 and x.shape[-1] == 512):
        return x
    return F.avg_pool2d(x[None], 2)[0]


def chain(pred, gt, sd, n_layers=5, dtype=torch.float64, down=True):
    """One image pair.  Returns a dict: loss, grad (dL/dpred), taps / taps_t (source / target, (C,h,w)), pre (source
    pre-activations), pool_in (source pool inputs), all in `dtype`."""
    nc = TAPS[n_layers - 1] + 1
    pairs = [(w.to(dtype), b.to(dtype)) for w, b in pairs_of(sd, nc)]
    p = pred.detach().to(dtype).requires_grad_(True)
    s, t = downsize(p, down), downsize(gt.detach().to(dtype), down)
    out = {"taps": [], "taps_t": [], "pre": [], "pool_in": [], "tap_loss": []}
    loss = 0
    for i, (w, b) in enumerate(pairs):
        if i in POOL_BEFORE:
            out["pool_in"].append(s.detach())
            s, t = F.max_pool2d(s[None], 2)[0], F.max_pool2d(t[None], 2)[0]
        pre = F.conv2d(s[None], w, b, padding=1)[0]
        out["pre"].append(pre.detach())
        s = F.relu(pre)
        with torch.no_grad():
            t = F.relu(F.conv2d(t[None], w, b, padding=1)[0])
        if i in TAPS:
            out["taps"].append(s.detach())
            out["taps_t"].append(t)
            li = (s - t).abs().mean()
            out["tap_loss"].append(li.detach())
            loss = loss + li
    out["loss"] = loss.detach()
    out["grad"] = torch.autograd.grad(loss, p)[0]
    return out


def maxerr(a32, a64):
    return float((a32.double() - a64).abs().max())


def e32_rel(a32, a64):
    """The float32 evaluation's max error against float64, relative to max |a64|."""
    m = float(a64.abs().max())
    return maxerr(a32, a64) / m if m > 0 else 0.0


def qualify(pred, gt, sd, n_layers=5, factor=16.0):
    """A seed qualifies if no decision of the gradient can flip inside the device's allowance: in float64 every source ReLU
    pre-activation, every pool top-two gap with a positive maximum, and every |source - target| at a tap with a non-zero
    feature is >= factor x the float32 evaluation's max error of that quantity.  Returns (ok, worst margin / error ratio)."""
    r64, r32 = chain(pred, gt, sd, n_layers, torch.float64), chain(pred, gt, sd, n_layers, torch.float32)
    worst = float("inf")
    for a64, a32 in zip(r64["pre"], r32["pre"]):
        worst = min(worst, float(a64.abs().min()) / max(maxerr(a32, a64), 1e-300))
    for a64, a32 in zip(r64["pool_in"], r32["pool_in"]):
        C, H, W = a64.shape
        win = a64[:, :H // 2 * 2, :W // 2 * 2].reshape(C, H // 2, 2, W // 2, 2).permute(0, 1, 3, 2, 4).reshape(C, H // 2, W // 2, 4)
        top = win.sort(dim=-1, descending=True).values
        gap = (top[..., 0] - top[..., 1])[top[..., 0] > 0]
        if gap.numel():
            worst = min(worst, float(gap.min()) / max(maxerr(a32, a64), 1e-300))
    for s64, t64, s32, t32 in zip(r64["taps"], r64["taps_t"], r32["taps"], r32["taps_t"]):
        d = (s64 - t64).abs()[(s64 != 0) | (t64 != 0)]
        if d.numel():
            worst = min(worst, float(d.min()) / max(maxerr(s32 - t32, s64 - t64), 1e-300))
    return worst >= factor, worst


# ---- single operations, channels-last in and out like the device's wrappers ------------------------------------------

def conv3x3_relu(x_hwc, w, b, relu=True):
    y = F.conv2d(x_hwc.permute(2, 0, 1)[None], w.to(x_hwc.dtype), None if b is None else b.to(x_hwc.dtype), padding=1)[0]
    return (F.relu(y) if relu else y).permute(1, 2, 0).contiguous()


def conv3x3_relu_bwd(gy_hwc, y_hwc, w):
    g = (gy_hwc * (y_hwc > 0)).permute(2, 0, 1)[None]
    return F.conv_transpose2d(g, w.to(gy_hwc.dtype), padding=1)[0].permute(1, 2, 0).contiguous()


def maxpool2(x_hwc):
    return F.max_pool2d(x_hwc.permute(2, 0, 1)[None], 2)[0].permute(1, 2, 0).contiguous()


def maxpool2_bwd(x_hwc, gy_hwc):
    x = x_hwc.detach().clone().requires_grad_(True)
    (maxpool2(x) * gy_hwc).sum().backward()
    return x.grad


def box_down2(img_chw, down=True):
    return (F.interpolate(img_chw[None], scale_factor=0.5, mode="bilinear")[0] if down else img_chw).permute(1, 2, 0).contiguous()


def box_down2_bwd(g_hwc, H, W, down=True):
    x = torch.zeros(g_hwc.shape[2], H, W, dtype=g_hwc.dtype, requires_grad=True)
    (box_down2(x, down) * g_hwc).sum().backward()
    return x.grad


def excess(a, b, rel, floor_rel):
    """max of |a - b| - (rel |b| + floor_rel max|b|): <= 0 passes."""
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float(((a - b).abs() - (rel * b.abs() + floor_rel * b.abs().max())).max())
