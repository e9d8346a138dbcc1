"""Float64 numpy oracle of the evaluation tail (d3ga_amd/evaluation.py, csrc/eval.hip): the target composition of the
reference's test.py:140-141,151, the RGBA ground truth of :186-187, the jet error heat map of recorder/heatmap.py:16-61 and
the PSNR of utils/image_utils.py:20-22.  The jet table is rebuilt here from the colormap's piecewise-linear segments the way
matplotlib builds its lookup table, independently of the library's compile-time table; matplotlib itself is only needed by
`reference_sequence`, the restatement of the reference's per-frame host detour that tools/time_eval.py times."""
import numpy as np

JET_SEGMENTS = {
    "r": [(0, 0), (.35, 0), (.66, 1), (.89, 1), (1, .5)],
    "g": [(0, 0), (.125, 0), (.375, 1), (.64, 1), (.91, 0), (1, 0)],
    "b": [(0, .5), (.11, 1), (.34, 1), (.65, 0), (1, 0)],
}
BAD = 256                      # row of the "bad" colour (a NaN error): transparent black
EDGE = 4e-7                    # float32 error of e: three squares, two adds and a square root on e <= 1.8 (3 * 2^-24 * 1.8 = 3.2e-7)


def jet_table_ref():
    """(257,3) uint8: matplotlib's 256-entry jet lookup table times 255, truncated (dist_to_rgb), plus the bad colour."""
    N = 256
    xind = (N - 1) * np.linspace(0, 1, N)
    cols = []
    for key in "rgb":
        d = np.array(JET_SEGMENTS[key], dtype=np.float64)
        x, y = d[:, 0] * (N - 1), d[:, 1]
        ind = np.searchsorted(x, xind)[1:-1]
        t = (xind[1:-1] - x[ind - 1]) / (x[ind] - x[ind - 1])
        lut = np.concatenate([[y[0]], t * (y[ind] - y[ind - 1]) + y[ind - 1], [y[-1]]])
        cols.append((np.clip(lut, 0, 1) * 255).astype(np.uint8))
    return np.concatenate([np.stack(cols, 1), np.zeros((1, 3), np.uint8)])


def heat_bins(e):
    """bin of the jet table for errors e (any float dtype): min(int(min(e, 1) 256), 255); NaN -> BAD."""
    e = np.asarray(e)
    nan = np.isnan(e)
    m = np.minimum(np.where(nan, 0, e), 1.0)
    return np.where(nan, BAD, np.minimum((m * 256).astype(np.int64), 255))


def bin_is_decided(e64):
    """True where a float32 evaluation of e must land in the same bin as the float64 one: e exactly 0, e >= 1 + EDGE, or
    e farther than EDGE from every multiple of 1/256 (tests: the remaining pixels may differ by one bin)."""
    e = np.asarray(e64, dtype=np.float64)
    k = np.round(e * 256.0) / 256.0
    return (e == 0) | (e >= 1 + EDGE) | ((np.abs(e - k) > EDGE) & (e < 1))


def compose_ref(image, alpha, boundary_fg, bg):
    """test.py:140-141,151,186-187 in float64 -> (target (...,3,H,W), ground_truth (...,4,H,W))."""
    image = np.asarray(image, dtype=np.float64)
    H, W = image.shape[-2:]
    lead = image.shape[:-3]
    alpha = np.asarray(alpha, dtype=np.float64).reshape(lead + (-1, H, W))
    a = alpha[..., 0:1, :, :] * (1.0 - np.asarray(boundary_fg).astype(np.float64).reshape(lead + (1, H, W)))
    fg = image * a
    return fg + (1.0 - a) * float(bg), np.concatenate([fg, a], axis=-3)


def errors_ref(target, pred):
    """e (...,H,W) in float64."""
    d = np.asarray(target, dtype=np.float64) - np.asarray(pred, dtype=np.float64)
    return np.sqrt((d * d).sum(axis=-3))


def heatmap_ref(target, pred, table=None):
    """(heat (...,3,H,W) float32 = table[bin] / 255 in float32, bins, e)."""
    table = jet_table_ref() if table is None else table
    e = errors_ref(target, pred)
    bins = heat_bins(e)
    heat = table[bins].astype(np.float32) / np.float32(255)
    return np.moveaxis(heat, -1, -3), bins, e


def psnr_channels_ref(target, pred):
    """20 log10(1 / sqrt(mse_c)) per channel in float64, (...,3); mse_c = 0 -> +inf."""
    d = np.asarray(target, dtype=np.float64) - np.asarray(pred, dtype=np.float64)
    mse = (d * d).mean(axis=(-2, -1))
    with np.errstate(divide="ignore"):
        return 20.0 * np.log10(1.0 / np.sqrt(mse))


def psnr_ref(target, pred):
    """The mean of the per-channel PSNRs: psnr(fake, target).mean() of recorder/heatmap.py:39."""
    return psnr_channels_ref(target, pred).mean(axis=-1)


def psnr_pooled_ref(target, pred):
    """The PSNR of the error pooled over the channels: what the metric is NOT."""
    d = np.asarray(target, dtype=np.float64) - np.asarray(pred, dtype=np.float64)
    return 20.0 * np.log10(1.0 / np.sqrt((d * d).mean(axis=(-3, -2, -1))))


def make_pair(seed, H, W, spread=0.25, B=None):
    """A seeded (gt, pred) pair as tools/gen_golden.py's gen_losses builds them: gt = rand, pred = clamp(gt + spread randn)."""
    rng = np.random.default_rng(seed)
    shape = (3, H, W) if B is None else (B, 3, H, W)
    gt = rng.random(shape).astype(np.float32)
    pred = np.clip(gt + spread * rng.standard_normal(shape), 0, 1).astype(np.float32)
    return gt, pred


def make_frame_inputs(seed, B, H, W, alpha_channels=1):
    """(pred, image, alpha, boundary_fg uint8) for the composition: alpha with exact 0s and 1s, a boundary band.  pred stays
    strictly inside (0, 1): a prediction clipped to 0 or 1 in front of a background pixel gives e = 1 EXACTLY, which float32
    gets right but which the tests' edge rule counts against the share of pixels it may excuse."""
    rng = np.random.default_rng(seed)
    image, pred = make_pair(seed + 1, H, W, B=B)
    pred = np.clip(pred, np.float32(0.004), np.float32(0.996))
    alpha = rng.random((B, alpha_channels, H, W)).astype(np.float32)
    alpha[rng.random(alpha.shape) < 0.2] = 0.0
    alpha[rng.random(alpha.shape) < 0.2] = 1.0
    boundary = (rng.random((B, 1, H, W)) < 0.15).astype(np.uint8)
    return pred, image, alpha, boundary


def reference_sequence(target, fake, ssim_fn, to_device):
    """The reference's compute_errors (recorder/heatmap.py:37-49) without LPIPS, on device tensors, step by step: two torch
    metrics with an .item() each, both images to the host, the numpy norm, matplotlib's ScalarMappable, the upload.
    ssim_fn(fake, target) -> 0-dim tensor; to_device(cpu tensor) -> device tensor."""
    import matplotlib as mpl
    import matplotlib.cm as cm
    import torch
    s = ssim_fn(fake, target).mean().item()
    mse = ((fake - target) ** 2).view(fake.shape[0], -1).mean(1, keepdim=True)
    p = (20 * torch.log10(1.0 / torch.sqrt(mse))).mean().item()
    t = target.permute(1, 2, 0).cpu().numpy()
    f = fake.permute(1, 2, 0).cpu().numpy()
    errors = np.linalg.norm(t - f, axis=2, keepdims=True, ord=2)
    h, w, _ = errors.shape
    errors = np.clip(0, 1.0, errors).reshape(h * w)
    mapper = cm.ScalarMappable(norm=mpl.colors.Normalize(vmin=0.0, vmax=1.0), cmap=mpl.colormaps["jet"])
    heat = mapper.to_rgba(errors)[:, 0:3].reshape(h, w, 3)
    heat = np.minimum(np.maximum(heat * 255, 0), 255).astype(np.uint8)
    return to_device(torch.from_numpy(heat)).permute(2, 0, 1) / 255, s, p


# (seed, B, H, W) of the GPU tests (tests/test_gpu_evaluation.py): W not a multiple of 4 and the pixel-by-pixel path, the quad
# path, W smaller than a wavefront, three workgroups per frame (9170 pixels / 4096) and frames with different content.
# tests/test_evaluation_host.py checks on the CPU that float32 numpy meets the heat map's edge rule on exactly these inputs.
GPU_CASES = [(101, 1, 5, 7), (102, 2, 33, 16), (103, 3, 70, 131), (104, 1, 64, 96)]
EXCUSED = 1e-3                 # at most this share of a case's pixels may sit within EDGE of a bin edge


def check_heat(heat, target64, pred64, table=None):
    """The heat map's rule: bit-identical to table[bin] / 255 on every decided pixel, at most one bin off on the others, and
    at most EXCUSED of the pixels undecided.  heat (...,3,H,W) float32; -> (number undecided, number of pixels)."""
    table = jet_table_ref() if table is None else table
    want, bins, e = heatmap_ref(target64, pred64, table)
    decided = bin_is_decided(e) | np.isnan(e)
    lut = table.astype(np.float32) / np.float32(255)
    got = np.moveaxis(np.asarray(heat), -3, -1)
    exact = (got == lut[bins]).all(-1)
    assert exact[decided].all(), f"{(~exact[decided]).sum()} decided pixels differ"
    near = exact | (got == lut[np.clip(bins - 1, 0, 255)]).all(-1) | (got == lut[np.clip(bins + 1, 0, 255)]).all(-1)
    assert near.all(), "a pixel is more than one bin off"
    n_open = int((~decided).sum())
    assert n_open <= EXCUSED * decided.size, f"{n_open} of {decided.size} pixels within {EDGE} of a bin edge"
    return n_open, decided.size
