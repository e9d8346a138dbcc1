"""Oracle of the LPIPS (VGG) metric (d3ga_amd/lpips.py): a restatement in plain torch on the CPU, in any dtype (float64 is the
yardstick, float32 gives e32, the float32 evaluation's own error).  The `lpips` package is not available here and the
reference tree holds no LPIPS code, so this is written from the paper and from recall of the public package (parity
unpinned): the scaling layer, the VGG16 chain, normalize_tensor with eps = 1e-10 ADDED TO THE NORM, the squared
difference, the 1x1 `lin` without bias, the spatial mean and the sum over the five taps.  tests/test_lpips_host.py pins the
distance itself to first-principles answers, independent of recall."""
import torch
import torch.nn.functional as F

CONV_KEYS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)      # torchvision vgg16().features
POOL_BEFORE = (2, 4, 7, 10)
TAPS = (1, 3, 6, 9, 12)
SLICE_OF = (1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5)                # the package's net.slice{s} each convolution sits in
VGG16_WIDTHS = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
SHIFT, SCALE = (-.030, -.088, -.188), (.458, .448, .450)
EPS = 1e-10


def make_weights(widths, seed, layout="torchvision", lins="lin"):
    """Seeded float32 state dict: He-initialised convolutions, biases uniform in +-0.1, heads uniform in [0, 0.2) with ONE
    NEGATIVE entry each.  layout "torchvision": features.K.*; "package": net.slice{s}.K.*.  lins "lin": lin{t}.model.1.weight;
    "lins": lins.t.model.1.weight.  The tensors do not depend on the layout."""
    g = torch.Generator().manual_seed(3000 + seed)
    sd, cin = {}, 3
    for k, s, c in zip(CONV_KEYS, SLICE_OF, widths):
        pre = f"features.{k}" if layout == "torchvision" else f"net.slice{s}.{k}"
        sd[pre + ".weight"] = torch.randn(c, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
        sd[pre + ".bias"] = (torch.rand(c, generator=g) - 0.5) * 0.2
        cin = c
    for t, i in enumerate(TAPS):
        l = torch.rand(widths[i], generator=g) * 0.2
        l[t % widths[i]] = -0.05
        sd[(f"lin{t}" if lins == "lin" else f"lins.{t}") + ".model.1.weight"] = l.view(1, -1, 1, 1)
    return sd


def pairs_of(sd):
    out = []
    for k, s in zip(CONV_KEYS, SLICE_OF):
        pre = f"features.{k}" if f"features.{k}.weight" in sd else f"net.slice{s}.{k}"
        out.append((sd[pre + ".weight"], sd[pre + ".bias"]))
    return out


def lins_of(sd):
    return [sd[f"lin{t}.model.1.weight"] if f"lin{t}.model.1.weight" in sd else sd[f"lins.{t}.model.1.weight"] for t in range(5)]


def scale_input(x, normalize=False):
    """(..., 3, H, W) -> the scaling layer's output, same layout."""
    if normalize:
        x = 2 * x - 1
    shift = torch.tensor(SHIFT, dtype=x.dtype).view(3, 1, 1)
    scale = torch.tensor(SCALE, dtype=x.dtype).view(3, 1, 1)
    return (x - shift) / scale


def normalize_tensor(f):
    """(N, C, h, w) -> unit vectors along C, eps added to the norm."""
    return f / (f.pow(2).sum(dim=1, keepdim=True).sqrt() + EPS)


def tap_distance(a, b, lin):
    """Features a, b (N, C, h, w), lin (C,) or (1, C, 1, 1) -> d (N, h, w): the 1x1 convolution without bias of the squared
    difference of the unit vectors."""
    d = (normalize_tensor(a) - normalize_tensor(b)) ** 2
    return (d * lin.to(a.dtype).reshape(1, -1, 1, 1)).sum(dim=1)


def features(x, sd):
    """The five taps (N, C, h, w) of scaled images x (N, 3, H, W), in x's dtype."""
    taps, s = [], x
    for i, (w, b) in enumerate(pairs_of(sd)):
        if i in POOL_BEFORE:
            s = F.max_pool2d(s, 2)
        s = F.relu(F.conv2d(s, w.to(x.dtype), b.to(x.dtype), padding=1))
        if i in TAPS:
            taps.append(s)
    return taps


def chain(fake, target, sd, normalize=False, dtype=torch.float64):
    """fake, target (B, 3, H, W) -> {"taps_a", "taps_b": five (B, C, h, w); "maps": five (B, h, w); "value": (B,)} in `dtype`."""
    fa = features(scale_input(fake.to(dtype), normalize), sd)
    fb = features(scale_input(target.to(dtype), normalize), sd)
    maps = [tap_distance(a, b, l) for a, b, l in zip(fa, fb, lins_of(sd))]
    return {"taps_a": fa, "taps_b": fb, "maps": maps, "value": sum(m.mean(dim=(1, 2)) for m in maps)}


# Seeds of the end-to-end cases (weights make_weights(widths, s), images perceptual_ref.make_images(H, W, s)) at the sizes
# tests/test_gpu_lpips.py uses.  The device's bar is 4 e32 per map, and e32 is a MAX statistic of one float32 evaluation.  A
# unit vector f / |f| amplifies the chain's error by 1 / |f|, so a map's largest error sits at its few pixels of small norm
# (norms of 0.04 against a median of 3 occur), or, for the last tap of a 16 x 16 image, at its only pixel: e32 is then one
# draw of a rounding error, not an estimate of its size, and ANOTHER float32 evaluation of this very oracle lands anywhere
# from 0.2 to 4 times it.  A seed qualifies if e32 is a usable yardstick for every map, decided from the oracle alone
# (test_lpips_host.py asserts it for every listed seed):
#   * e32 >= 2^-24, the rounding of merely storing the map's largest value in float32;
#   * QUALIFY_ORDERS further float32 evaluations of the oracle, the convolutions summed in other orders (features_reordered),
#     all stay within QUALIFY_SPREAD e32: half of the device's factor 4 is left to the device's own arithmetic (three bf16
#     pieces per operand, sums in chunks of 128 k).
NARROW_SIZES = ((16, 16), (37, 53), (40, 56))
# {size: {normalize: seeds}}: the first two seeds (from 0) that qualify with a spread of at most 1.7 where this was written: the room
# up to QUALIFY_SPREAD is for another CPU's float32 sums
NARROW_SEEDS = {(16, 16): {False: (2, 19), True: (5, 8)}, (37, 53): {False: (6, 13), True: (6, 13)}, (40, 56): {False: (5, 6), True: (5, 6)}}
VGG16_CASE = ((32, 32), 2)
QUALIFY_ORDERS, QUALIFY_SPREAD = 4, 2.0


def features_reordered(x, sd, order):
    """features() in x's dtype with every convolution as im2col + matmul, K permuted by the seed `order` and summed in chunks
    of 128: the same arithmetic in another order."""
    g = torch.Generator().manual_seed(7000 + order)
    taps, s = [], x
    for i, (w, b) in enumerate(pairs_of(sd)):
        if i in POOL_BEFORE:
            s = F.max_pool2d(s, 2)
        N, _, H, W = s.shape
        cols = F.unfold(s, 3, padding=1)                           # (N, 9 Cin, H W)
        K = cols.shape[1]
        perm, wm = torch.randperm(K, generator=g), w.to(x.dtype).reshape(w.shape[0], K)
        acc = torch.zeros(N, w.shape[0], H * W, dtype=x.dtype)
        for k0 in range(0, K, 128):
            idx = perm[k0:k0 + 128]
            acc = acc + wm[:, idx] @ cols[:, idx]
        s = F.relu(acc + b.to(x.dtype).view(1, -1, 1)).view(N, -1, H, W)
        if i in TAPS:
            taps.append(s)
    return taps


def qualify(widths, H, W, seed, normalize):
    """(qualifies, smallest e32 in units of 2^-24, largest reordered error / e32) for one seeded case."""
    import perceptual_ref as pr
    sd = make_weights(widths, seed)
    f, t = pr.make_images(H, W, seed, n=1)
    r64, r32 = chain(f, t, sd, normalize), chain(f, t, sd, normalize, torch.float32)
    e32 = [e32_rel(a, b) for a, b in zip(r32["maps"], r64["maps"])]
    spread = 0.0
    for order in range(QUALIFY_ORDERS):
        fa = features_reordered(scale_input(f, normalize), sd, 2 * order)
        fb = features_reordered(scale_input(t, normalize), sd, 2 * order + 1)
        for a, b, l, m64, e in zip(fa, fb, lins_of(sd), r64["maps"], e32):
            spread = max(spread, e32_rel(tap_distance(a, b, l), m64) / max(e, 1e-300))
    floor = min(e32) * 2.0 ** 24
    return floor >= 1.0 and spread <= QUALIFY_SPREAD, floor, spread


def maxerr(a32, a64):
    return float((a32.double() - a64).abs().max())


def e32_rel(a32, a64):
    """The float32 evaluation's max error against float64, relative to max |a64|."""
    m = float(a64.abs().max())
    return maxerr(a32, a64) / m if m > 0 else 0.0
