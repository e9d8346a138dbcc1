"""TEST INFRASTRUCTURE ONLY -- the per-pixel oracle of the image losses (csrc/loss.hip) and the table of cases.

`maps(a, b, dtype)` evaluates the SSIM of oracle/losses.py in plain torch on the CPU and also returns what the device keeps
between its forward and its backward: the three maps Dm, Dq1, Dq12 (d ssim / d(w*x), d(w*x^2), d(w*xy) per pixel) and the
gradient of the mean assembled from them, (w*Dm + 2 a (w*Dq1) + b (w*Dq12)) / n.  The window is oracle/losses.py's: the
float32 1-D window, its 2-D product rounded to float32, THEN cast to `dtype` -- with it the float64 gradient equals autograd
through oracle.losses.ssim to 1e-12 (tests/test_losses_host.py); a window that is separable in float64 agrees only to 1e-8.

One function, two dtypes: float64 is the oracle, float32 its twin.  `bar(q64, q32)` turns the twin's own deviation into the
bar of a case and a quantity, on the spot:  8 max|q32 - q64| + 8 2^-23 max|q64|.  The device does the same float32
arithmetic in another order (11 + 11 separable taps instead of 121, fma), which `maps_separable32` restates on the CPU;
test_losses_host.py holds it under the bar at every case.  The second term is the floor for cases where float32 torch is
exact (constant images): two 1-ulp reciprocals and up to six roundings in A B iD iE.  No pixel is left out anywhere.
"""
import collections

import torch
import torch.nn.functional as F

from oracle.losses import gaussian_window

EPS32 = 2.0 ** -23
C1, C2 = 0.01 ** 2, 0.03 ** 2
L1_VALUE_BAR = 1e-6                      # absolute, the bar of test_losses_fuzz
SUM_ORDER_REL = 1e-6                     # two runs of the same atomic sum (test_gpu_perceptual.py)

# csrc/loss.hip, mirrored as plain integers (tests/test_losses_host.py derives every claim of CASES from them)
MARCH_USE = 244                          # kMarchUse: output columns of a strip
TILE_W, TILE_H = 16, 32                  # kSsimTW, kSsimTH
GROUP = 4                                # rows per group of the marching kernels
SEG16 = 16                               # the smallest seg_rows (every launch with more items than the device has slots)
CAP_TILED_FWD, CAP_MARCH_FWD, CAP_BWD = 2048, 4096, 8192   # kSsimTiledFwdGrid, kSsimMarchFwdGrid, kSsimBwdGrid
L1_BLOCK, L1_CAP_ATOMIC, L1_CAP = 256, 512, 2048

Maps = collections.namedtuple("Maps", "val Dm Dq1 Dq12 grad_ssim grad_l1")
QUANTITIES = ("Dm", "Dq1", "Dq12")


def window2d(dtype):
    w1 = gaussian_window().unsqueeze(1)
    return w1.mm(w1.t()).float().to(dtype)


def _conv2d(t, win):
    """Depthwise 11x11, zero padding 5, of a (C,H,W) stack (the channels as a batch: one window for all)."""
    return F.conv2d(t.unsqueeze(1), win[None, None], padding=5).squeeze(1)


def _conv_sep(t, w1):
    """The same as 11 vertical then 11 horizontal taps (the device's order)."""
    t = F.conv2d(t.unsqueeze(1), w1.view(1, 1, 11, 1), padding=(5, 0))
    return F.conv2d(t, w1.view(1, 1, 1, 11), padding=(0, 5)).squeeze(1)


def _maps(a, b, conv):
    n = a.numel()
    mu1, mu2 = conv(a), conv(b)
    s1, s2, s12 = conv(a * a) - mu1 * mu1, conv(b * b) - mu2 * mu2, conv(a * b) - mu1 * mu2
    A, B = 2 * mu1 * mu2 + C1, 2 * s12 + C2
    D, E = mu1 * mu1 + mu2 * mu2 + C1, s1 + s2 + C2
    val = A * B / (D * E)
    Dq1 = -val / E
    Dq12 = 2 * A / (D * E)
    d_mu1 = 2 * mu2 * B / (D * E) - 2 * mu1 * val / D
    Dm = d_mu1 - 2 * mu1 * Dq1 - mu2 * Dq12
    grad_ssim = (conv(Dm) + 2 * a * conv(Dq1) + b * conv(Dq12)) / n
    grad_l1 = torch.sign(a - b) / n
    return Maps(val, Dm, Dq1, Dq12, grad_ssim, grad_l1)


def maps(a, b, dtype):
    """val, Dm, Dq1, Dq12 per pixel, grad_ssim = d mean(val) / d a and grad_l1 = sign(a - b) / n of two (C,H,W) float32 images,
    evaluated in `dtype`.  sign() sees the float32 inputs in every dtype: exact ties are exact everywhere."""
    win = window2d(dtype)
    return _maps(a.to(dtype), b.to(dtype), lambda t: _conv2d(t, win))


def maps_separable32(a, b):
    """maps() in float32 with the window applied as two 1-D passes: the summation order of the device kernels."""
    w1 = gaussian_window()
    return _maps(a.float(), b.float(), lambda t: _conv_sep(t, w1))


def bar(q64, q32):
    return 8.0 * float((q32.double() - q64).abs().max()) + 8.0 * EPS32 * float(q64.abs().max())


def bar_mean_ssim(val64, val32):
    return 8.0 * float((val32.double() - val64).abs().mean()) + 8.0 * EPS32


KINDS = ("noise", "white", "binary", "same", "hdr")


def make_images(kind, C, H, W, seed):
    """(a, b) float32 (C,H,W): b = rand, a = clamp(b + 0.3 randn, 0, 1), then
    noise as is; white: both exactly 1.0 outside a centred ellipse with semi-axes H/3, W/3 (a figure on a white background);
    binary: both thresholded at 0.5 and the first H // 2 rows of both 1.0 (the silhouette pass); same: a = b; hdr: a <- 4 a - 0.5
    (an unclamped render)."""
    g = torch.Generator().manual_seed(seed)
    b = torch.rand(C, H, W, generator=g)
    a = (b + 0.3 * torch.randn(C, H, W, generator=g)).clamp(0, 1)
    if kind == "white":
        y = (torch.arange(H, dtype=torch.float64) - (H - 1) / 2).view(H, 1) / (H / 3)
        x = (torch.arange(W, dtype=torch.float64) - (W - 1) / 2).view(1, W) / (W / 3)
        outside = (x * x + y * y > 1.0).expand(C, H, W)
        a, b = a.masked_fill(outside, 1.0), b.masked_fill(outside, 1.0)
    elif kind == "binary":
        a, b = (a > 0.5).float(), (b > 0.5).float()
        a[:, : H // 2], b[:, : H // 2] = 1.0, 1.0
    elif kind == "same":
        a = b.clone()
    elif kind == "hdr":
        a = 4 * a - 0.5
    elif kind != "noise":
        raise ValueError(kind)
    return a.contiguous(), b.contiguous()


def ceil_div(a, b):
    return -(-a // b)


def l1_partials(n, cap=L1_CAP):
    """Workgroups (= partial sums) of an l1_mean launch over n elements: loss_grid(n / 4, cap)."""
    return max(1, min(ceil_div(n // 4, L1_BLOCK), cap))


class Case(collections.namedtuple("Case", "kind C H W why strips last tiles segs16 w4 h4 hrel over")):
    """One image shape and class, and what it is there for.  Every field behind `why` is a CLAIM about the shape, checked
    against the mirrored constants by tests/test_losses_host.py (a case that stops exercising its seam fails there):
      strips   marching strips of 244 output columns;  last: output columns of the last strip (1: a strip of one column,
               5: one halo wide)
      tiles    16 x 32 tiles per channel;  segs16: segments per strip at seg_rows = 16
      w4, h4   W % 4 (0: the 16-byte stores) and H % 4 (rows of the last group; 0: four)
      hrel     H against 4, 14 and 16: one group / the 14-row register window (H >= 10: the first prefetch brings image rows)
               / one segment
      over     the grid caps the launch exceeds, so that its persistent loop iterates: tf tiled forward (C tiles > 2048),
               mf marching forward (C strips ceil(H / 128) > 4096: the fewest items any seg_rows in 16..128 gives; H <= 16 in
               the cap cases, one segment whatever the search picks), tb / mb the backward kernels (> 8192); "-": none."""
    __slots__ = ()

    def __new__(cls, kind, C, H, W, why, **claims):
        return super().__new__(cls, kind, C, H, W, why, **claims)

    @property
    def id(self):
        return f"{self.kind}-{self.C}x{self.H}x{self.W}"

    @property
    def seed(self):
        return 1000 * self.H + self.W + 7 * self.C


def make_case(case):
    return make_images(case.kind, case.C, case.H, case.W, case.seed)


# Every shape runs with the noise class (bars of about 1e-5 of max: one dropped edge tap, weight 1.0e-3, stands out);
# C in {1, 2, 3} spread over them.  Then the items above the grid caps (tiny images, many channels), two shapes with
# H > 128 = the largest segment and C ceil(H / 16) far above CUs x resident workgroups (the cost search of ssim_march_rows
# moves away from 16 rows, and at least two segments exist whatever it picks), and the workload's image classes at four shapes.
CASES = [
    Case("noise", 2, 9, 1, "narrow", strips=1, last=1, tiles=1, segs16=1, w4=1, h4=1, hrel="><<", over="-"),
    Case("noise", 3, 9, 2, "narrow", strips=1, last=2, tiles=1, segs16=1, w4=2, h4=1, hrel="><<", over="-"),
    Case("noise", 1, 9, 3, "narrow", strips=1, last=3, tiles=1, segs16=1, w4=3, h4=1, hrel="><<", over="-"),
    Case("noise", 2, 9, 4, "narrow", strips=1, last=4, tiles=1, segs16=1, w4=0, h4=1, hrel="><<", over="-"),
    Case("noise", 3, 9, 5, "narrow", strips=1, last=5, tiles=1, segs16=1, w4=1, h4=1, hrel="><<", over="-"),
    Case("noise", 1, 9, 7, "narrow", strips=1, last=7, tiles=1, segs16=1, w4=3, h4=1, hrel="><<", over="-"),
    Case("noise", 2, 9, 8, "narrow", strips=1, last=8, tiles=1, segs16=1, w4=0, h4=1, hrel="><<", over="-"),
    Case("noise", 3, 9, 11, "narrow", strips=1, last=11, tiles=1, segs16=1, w4=3, h4=1, hrel="><<", over="-"),
    Case("noise", 1, 9, 12, "narrow", strips=1, last=12, tiles=1, segs16=1, w4=0, h4=1, hrel="><<", over="-"),
    Case("noise", 2, 9, 15, "tile-x", strips=1, last=15, tiles=1, segs16=1, w4=3, h4=1, hrel="><<", over="-"),
    Case("noise", 3, 9, 16, "tile-x", strips=1, last=16, tiles=1, segs16=1, w4=0, h4=1, hrel="><<", over="-"),
    Case("noise", 1, 9, 17, "tile-x", strips=1, last=17, tiles=2, segs16=1, w4=1, h4=1, hrel="><<", over="-"),
    Case("noise", 2, 9, 31, "tile-x", strips=1, last=31, tiles=2, segs16=1, w4=3, h4=1, hrel="><<", over="-"),
    Case("noise", 3, 9, 32, "tile-x", strips=1, last=32, tiles=2, segs16=1, w4=0, h4=1, hrel="><<", over="-"),
    Case("noise", 1, 9, 33, "tile-x", strips=1, last=33, tiles=3, segs16=1, w4=1, h4=1, hrel="><<", over="-"),
    Case("noise", 2, 6, 243, "strip", strips=1, last=243, tiles=16, segs16=1, w4=3, h4=2, hrel="><<", over="-"),
    Case("noise", 3, 6, 244, "strip", strips=1, last=244, tiles=16, segs16=1, w4=0, h4=2, hrel="><<", over="-"),
    Case("noise", 1, 6, 245, "strip", strips=2, last=1, tiles=16, segs16=1, w4=1, h4=2, hrel="><<", over="-"),
    Case("noise", 2, 6, 248, "strip", strips=2, last=4, tiles=16, segs16=1, w4=0, h4=2, hrel="><<", over="-"),
    Case("noise", 3, 6, 249, "strip", strips=2, last=5, tiles=16, segs16=1, w4=1, h4=2, hrel="><<", over="-"),
    Case("noise", 1, 6, 253, "strip", strips=2, last=9, tiles=16, segs16=1, w4=1, h4=2, hrel="><<", over="-"),
    Case("noise", 2, 5, 488, "strips", strips=2, last=244, tiles=31, segs16=1, w4=0, h4=1, hrel="><<", over="-"),
    Case("noise", 3, 5, 489, "strips", strips=3, last=1, tiles=31, segs16=1, w4=1, h4=1, hrel="><<", over="-"),
    Case("noise", 1, 5, 733, "strips", strips=4, last=1, tiles=46, segs16=1, w4=1, h4=1, hrel="><<", over="-"),
    Case("noise", 2, 1, 6, "groups", strips=1, last=6, tiles=1, segs16=1, w4=2, h4=1, hrel="<<<", over="-"),
    Case("noise", 3, 2, 6, "groups", strips=1, last=6, tiles=1, segs16=1, w4=2, h4=2, hrel="<<<", over="-"),
    Case("noise", 1, 3, 6, "groups", strips=1, last=6, tiles=1, segs16=1, w4=2, h4=3, hrel="<<<", over="-"),
    Case("noise", 2, 4, 6, "groups", strips=1, last=6, tiles=1, segs16=1, w4=2, h4=0, hrel="=<<", over="-"),
    Case("noise", 3, 5, 6, "groups", strips=1, last=6, tiles=1, segs16=1, w4=2, h4=1, hrel="><<", over="-"),
    Case("noise", 1, 7, 6, "groups", strips=1, last=6, tiles=1, segs16=1, w4=2, h4=3, hrel="><<", over="-"),
    Case("noise", 2, 8, 6, "groups", strips=1, last=6, tiles=1, segs16=1, w4=2, h4=0, hrel="><<", over="-"),
    Case("noise", 3, 10, 6, "groups", strips=1, last=6, tiles=1, segs16=1, w4=2, h4=2, hrel="><<", over="-"),
    Case("noise", 1, 11, 6, "groups", strips=1, last=6, tiles=1, segs16=1, w4=2, h4=3, hrel="><<", over="-"),
    Case("noise", 2, 13, 6, "groups", strips=1, last=6, tiles=1, segs16=1, w4=2, h4=1, hrel="><<", over="-"),
    Case("noise", 3, 14, 6, "groups", strips=1, last=6, tiles=1, segs16=1, w4=2, h4=2, hrel=">=<", over="-"),
    Case("noise", 1, 15, 6, "groups", strips=1, last=6, tiles=1, segs16=1, w4=2, h4=3, hrel=">><", over="-"),
    Case("noise", 3, 16, 6, "segs", strips=1, last=6, tiles=1, segs16=1, w4=2, h4=0, hrel=">>=", over="-"),
    Case("noise", 1, 17, 6, "segs", strips=1, last=6, tiles=1, segs16=2, w4=2, h4=1, hrel=">>>", over="-"),
    Case("noise", 2, 18, 6, "segs", strips=1, last=6, tiles=1, segs16=2, w4=2, h4=2, hrel=">>>", over="-"),
    Case("noise", 3, 19, 6, "segs", strips=1, last=6, tiles=1, segs16=2, w4=2, h4=3, hrel=">>>", over="-"),
    Case("noise", 1, 20, 6, "segs", strips=1, last=6, tiles=1, segs16=2, w4=2, h4=0, hrel=">>>", over="-"),
    Case("noise", 2, 31, 6, "segs", strips=1, last=6, tiles=1, segs16=2, w4=2, h4=3, hrel=">>>", over="-"),
    Case("noise", 3, 32, 6, "segs", strips=1, last=6, tiles=1, segs16=2, w4=2, h4=0, hrel=">>>", over="-"),
    Case("noise", 1, 33, 6, "segs", strips=1, last=6, tiles=2, segs16=3, w4=2, h4=1, hrel=">>>", over="-"),
    Case("noise", 2, 63, 6, "segs", strips=1, last=6, tiles=2, segs16=4, w4=2, h4=3, hrel=">>>", over="-"),
    Case("noise", 3, 64, 6, "segs", strips=1, last=6, tiles=2, segs16=4, w4=2, h4=0, hrel=">>>", over="-"),
    Case("noise", 1, 65, 6, "segs", strips=1, last=6, tiles=3, segs16=5, w4=2, h4=1, hrel=">>>", over="-"),
    Case("noise", 2, 1, 20, "groups", strips=1, last=20, tiles=2, segs16=1, w4=0, h4=1, hrel="<<<", over="-"),
    Case("noise", 3, 2, 20, "groups", strips=1, last=20, tiles=2, segs16=1, w4=0, h4=2, hrel="<<<", over="-"),
    Case("noise", 1, 3, 20, "groups", strips=1, last=20, tiles=2, segs16=1, w4=0, h4=3, hrel="<<<", over="-"),
    Case("noise", 2, 4, 20, "groups", strips=1, last=20, tiles=2, segs16=1, w4=0, h4=0, hrel="=<<", over="-"),
    Case("noise", 3, 5, 20, "groups", strips=1, last=20, tiles=2, segs16=1, w4=0, h4=1, hrel="><<", over="-"),
    Case("noise", 1, 7, 20, "groups", strips=1, last=20, tiles=2, segs16=1, w4=0, h4=3, hrel="><<", over="-"),
    Case("noise", 2, 8, 20, "groups", strips=1, last=20, tiles=2, segs16=1, w4=0, h4=0, hrel="><<", over="-"),
    Case("noise", 3, 10, 20, "groups", strips=1, last=20, tiles=2, segs16=1, w4=0, h4=2, hrel="><<", over="-"),
    Case("noise", 1, 11, 20, "groups", strips=1, last=20, tiles=2, segs16=1, w4=0, h4=3, hrel="><<", over="-"),
    Case("noise", 2, 13, 20, "groups", strips=1, last=20, tiles=2, segs16=1, w4=0, h4=1, hrel="><<", over="-"),
    Case("noise", 3, 14, 20, "groups", strips=1, last=20, tiles=2, segs16=1, w4=0, h4=2, hrel=">=<", over="-"),
    Case("noise", 1, 15, 20, "groups", strips=1, last=20, tiles=2, segs16=1, w4=0, h4=3, hrel=">><", over="-"),
    Case("noise", 3, 16, 20, "segs", strips=1, last=20, tiles=2, segs16=1, w4=0, h4=0, hrel=">>=", over="-"),
    Case("noise", 1, 17, 20, "segs", strips=1, last=20, tiles=2, segs16=2, w4=0, h4=1, hrel=">>>", over="-"),
    Case("noise", 2, 18, 20, "segs", strips=1, last=20, tiles=2, segs16=2, w4=0, h4=2, hrel=">>>", over="-"),
    Case("noise", 3, 19, 20, "segs", strips=1, last=20, tiles=2, segs16=2, w4=0, h4=3, hrel=">>>", over="-"),
    Case("noise", 1, 20, 20, "segs", strips=1, last=20, tiles=2, segs16=2, w4=0, h4=0, hrel=">>>", over="-"),
    Case("noise", 2, 31, 20, "segs", strips=1, last=20, tiles=2, segs16=2, w4=0, h4=3, hrel=">>>", over="-"),
    Case("noise", 3, 32, 20, "segs", strips=1, last=20, tiles=2, segs16=2, w4=0, h4=0, hrel=">>>", over="-"),
    Case("noise", 1, 33, 20, "segs", strips=1, last=20, tiles=4, segs16=3, w4=0, h4=1, hrel=">>>", over="-"),
    Case("noise", 2, 63, 20, "segs", strips=1, last=20, tiles=4, segs16=4, w4=0, h4=3, hrel=">>>", over="-"),
    Case("noise", 3, 64, 20, "segs", strips=1, last=20, tiles=4, segs16=4, w4=0, h4=0, hrel=">>>", over="-"),
    Case("noise", 1, 65, 20, "segs", strips=1, last=20, tiles=6, segs16=5, w4=0, h4=1, hrel=">>>", over="-"),
    Case("noise", 2100, 3, 5, "cap", strips=1, last=5, tiles=1, segs16=1, w4=1, h4=3, hrel="<<<", over="tf"),
    Case("noise", 4100, 5, 7, "cap", strips=1, last=7, tiles=1, segs16=1, w4=3, h4=1, hrel="><<", over="tf+mf"),
    Case("noise", 8200, 3, 5, "cap", strips=1, last=5, tiles=1, segs16=1, w4=1, h4=3, hrel="<<<", over="tf+mf+tb+mb"),
    Case("noise", 700, 150, 6, "seg_rows", strips=1, last=6, tiles=5, segs16=10, w4=2, h4=2, hrel=">>>", over="tf"),
    Case("noise", 1500, 131, 4, "seg_rows", strips=1, last=4, tiles=5, segs16=9, w4=0, h4=3, hrel=">>>", over="tf"),
    Case("white", 3, 33, 245, "class", strips=2, last=1, tiles=32, segs16=3, w4=1, h4=1, hrel=">>>", over="-"),
    Case("white", 3, 70, 45, "class", strips=1, last=45, tiles=9, segs16=5, w4=1, h4=2, hrel=">>>", over="-"),
    Case("white", 1, 7, 5, "class", strips=1, last=5, tiles=1, segs16=1, w4=1, h4=3, hrel="><<", over="-"),
    Case("white", 2, 17, 489, "class", strips=3, last=1, tiles=31, segs16=2, w4=1, h4=1, hrel=">>>", over="-"),
    Case("binary", 3, 33, 245, "class", strips=2, last=1, tiles=32, segs16=3, w4=1, h4=1, hrel=">>>", over="-"),
    Case("binary", 3, 70, 45, "class", strips=1, last=45, tiles=9, segs16=5, w4=1, h4=2, hrel=">>>", over="-"),
    Case("binary", 1, 7, 5, "class", strips=1, last=5, tiles=1, segs16=1, w4=1, h4=3, hrel="><<", over="-"),
    Case("binary", 2, 17, 489, "class", strips=3, last=1, tiles=31, segs16=2, w4=1, h4=1, hrel=">>>", over="-"),
    Case("same", 3, 33, 245, "class", strips=2, last=1, tiles=32, segs16=3, w4=1, h4=1, hrel=">>>", over="-"),
    Case("same", 3, 70, 45, "class", strips=1, last=45, tiles=9, segs16=5, w4=1, h4=2, hrel=">>>", over="-"),
    Case("same", 1, 7, 5, "class", strips=1, last=5, tiles=1, segs16=1, w4=1, h4=3, hrel="><<", over="-"),
    Case("same", 2, 17, 489, "class", strips=3, last=1, tiles=31, segs16=2, w4=1, h4=1, hrel=">>>", over="-"),
    Case("hdr", 3, 33, 245, "class", strips=2, last=1, tiles=32, segs16=3, w4=1, h4=1, hrel=">>>", over="-"),
    Case("hdr", 3, 70, 45, "class", strips=1, last=45, tiles=9, segs16=5, w4=1, h4=2, hrel=">>>", over="-"),
    Case("hdr", 1, 7, 5, "class", strips=1, last=5, tiles=1, segs16=1, w4=1, h4=3, hrel="><<", over="-"),
    Case("hdr", 2, 17, 489, "class", strips=3, last=1, tiles=31, segs16=2, w4=1, h4=1, hrel=">>>", over="-"),
]
