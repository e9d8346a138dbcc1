#!/usr/bin/env python3
"""Generate tests/golden/eval_cases.npz -- and nothing else -- by running the reference's OWN evaluation code on the CPU:
utils.image_utils.psnr, utils.loss_utils.ssim, recorder.heatmap.dist_to_rgb, compute_heatmap and compute_errors.

Runs only where the reference checkout and matplotlib (one that still has `cm.get_cmap`, i.e. < 3.11) are present.  The
import-stub harness is tools/gen_golden.py's `install_harness`, with the real matplotlib let through; the stubbed `lpips`
package makes compute_errors' third metric a mock, so SSIM, PSNR and the heat map alone are recorded.

Cases:
  a, b, c   3x37x53, 3x16x16, 3x64x96: gt = rand, pred = clamp(gt + 0.25 randn, 0, 1), as gen_losses builds its pairs
  wide      3x24x40 with pred outside [0, 1], so that e > 1 occurs
  ramp      4001 errors over [0, 1.8] and their uint8 heat row (dist_to_rgb)
  edge      the errors 0, 1, just below and just above 1, and NaN, with their heat rows
  table     dist_to_rgb of the 256 bin centres: the reference's 256 x 3 uint8 jet table
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as gg  # noqa: E402

OUT = os.path.join(HERE, "..", "tests", "golden", "eval_cases.npz")


def main():
    gg.ABSENT.discard("matplotlib")
    gg.install_harness()
    warnings.filterwarnings("ignore", message=".*get_cmap.*")
    import matplotlib
    from recorder import heatmap as hm
    from utils import image_utils, loss_utils

    out = {"matplotlib_version": np.array(matplotlib.__version__)}
    g = torch.Generator().manual_seed(41)
    pairs = {}
    for name, (H, W) in {"a": (37, 53), "b": (16, 16), "c": (64, 96)}.items():
        gt = torch.rand(3, H, W, generator=g)
        pairs[name] = (gt, (gt + 0.25 * torch.randn(3, H, W, generator=g)).clamp(0, 1))
    gt = torch.rand(3, 24, 40, generator=g)
    pairs["wide"] = (gt, gt + 0.6 * torch.randn(3, 24, 40, generator=g))
    for name, (gt, pred) in pairs.items():
        heat, s, p, _ = hm.compute_errors(gt, pred)                       # (target, fake)
        heat2, p2 = hm.compute_heatmap(gt, pred)
        per_channel = image_utils.psnr(pred, gt)
        assert heat.shape == gt.shape and heat2.shape == (gt.shape[1], gt.shape[2], 3) and heat2.dtype == np.float32
        assert p == p2 and per_channel.shape == (3, 1) and abs(float(per_channel.mean()) - p) < 1e-6
        assert abs(float(loss_utils.ssim(pred, gt)) - s) < 1e-7
        assert np.array_equal(heat.permute(1, 2, 0).numpy(), heat2)       # uint8 / 255 in float32 == (uint8 / 255.0) as float32
        out.update({f"{name}_gt": gt.numpy(), f"{name}_pred": pred.numpy(), f"{name}_heat": heat.numpy(), f"{name}_heat_hwc": heat2,
                    f"{name}_ssim": np.float64(s), f"{name}_psnr": np.float64(p), f"{name}_psnr_channels": per_channel.numpy()})
    e = (pairs["wide"][0] - pairs["wide"][1]).norm(dim=0)
    assert float(e.max()) > 1.0

    def rows(errors):
        return hm.dist_to_rgb(np.asarray(errors).reshape(1, -1, 1))[0]

    ramp = np.linspace(0.0, 1.8, 4001).astype(np.float32)
    out["ramp"], out["ramp_heat"] = ramp, rows(ramp)
    one = np.float32(1)
    edge = np.array([0.0, 1.0, np.nextafter(one, np.float32(0)), np.nextafter(one, np.float32(2)), np.nan, 0.5, 1.0 / 256], dtype=np.float32)
    out["edge"], out["edge_heat"] = edge, rows(edge)
    centres = ((np.arange(256) + 0.5) / 256).astype(np.float32)
    out["table"] = rows(centres)
    assert out["table"].shape == (256, 3) and out["table"].dtype == np.uint8
    np.savez_compressed(OUT, **out)
    print("wrote", os.path.abspath(OUT), os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
