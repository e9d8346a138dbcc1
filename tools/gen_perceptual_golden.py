#!/usr/bin/env python3
"""Generate tests/golden/vgg_cases.npz -- and nothing else -- by running the reference's OWN `VGGLoss`
(utils/loss_utils.py:109-160) on the CPU.

Runs only where the reference checkout is present.  The import-stub harness is tools/gen_golden.py's `install_harness`;
`torchvision.models.vgg19` is bound to a stand-in that returns an `nn.Sequential` in VGG19's 37-module layout at narrow
widths (tests/perceptual_ref.py: GOLDEN_WIDTHS, seeded He weights), so that the weights fit the fixture.

Recorded:
  w.<key>                    the state dict of the stand-in (`features.K.weight` / `features.K.bias`)
  odd_* / even_*             pred, gt (3x37x53, 3x40x56) and, for n_layers 5 and 2, loss_n<k> and grad_n<k> = dL/dpred
  shape_<H>x<W>              the (h, w) that downsize + random_crop return for 512x512, 1024x1024, 1100x1300, 747x1022
"""
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import gen_golden as gg  # noqa: E402
import perceptual_ref as pr  # noqa: E402

OUT = os.path.join(HERE, "..", "tests", "golden", "vgg_cases.npz")
GOLDEN_SEED = pr.GOLDEN_SEED


def narrow_vgg19(widths, sd):
    """VGG19's `features`: 2, 2, 4, 4, 4 (conv, relu) pairs, a max pool behind each group: 37 modules."""
    mods, cin, i = [], 3, 0
    for group in (2, 2, 4, 4, 4):
        for _ in range(group):
            mods += [nn.Conv2d(cin, widths[i], 3, padding=1), nn.ReLU(inplace=True)]
            cin = widths[i]
            i += 1
        mods.append(nn.MaxPool2d(2, 2))
    # the stand-in has all 16 convolutions of VGG19; the three behind relu5_1 are never run and take the last width
    feats = nn.Sequential(*mods)
    assert len(feats) == 37
    feats.load_state_dict({k[len("features."):]: v for k, v in sd.items()}, strict=False)
    return feats


def main():
    gg.install_harness()
    from utils import loss_utils

    widths16 = list(pr.GOLDEN_WIDTHS) + [pr.GOLDEN_WIDTHS[-1]] * 3
    sd = pr.make_weights(pr.GOLDEN_WIDTHS, GOLDEN_SEED)
    stand_in = type("VGG", (), {})()
    loss_utils.models.vgg19 = lambda *a, **k: stand_in
    out = {"w." + k: v.numpy() for k, v in sd.items()}
    out["widths"] = np.array(pr.GOLDEN_WIDTHS, np.int32)
    cases = {"odd": (37, 53), "even": (40, 56)}
    for n_layers in (5, 2):
        stand_in.features = narrow_vgg19(widths16, sd)
        vl = loss_utils.VGGLoss(n_layers=n_layers)
        assert not any(p.requires_grad for p in vl.parameters())
        for name, (H, W) in cases.items():
            pred, gt = pr.make_images(H, W, GOLDEN_SEED + (0 if name == "odd" else 1))
            p = pred.clone().requires_grad_(True)
            g = gt.clone().requires_grad_(True)
            loss = vl(p[None], g[None])                                   # train.py:213
            loss.backward()
            assert g.grad is None or float(g.grad.abs().max()) == 0.0      # the target runs under no_grad
            out.update({f"{name}_pred": pred.numpy(), f"{name}_gt": gt.numpy(), f"{name}_loss_n{n_layers}": np.float64(loss.item()),
                        f"{name}_grad_n{n_layers}": p.grad.numpy()})
    for H, W in ((512, 512), (1024, 1024), (1100, 1300), (747, 1022)):
        x = torch.zeros(1, 3, H, W)
        a, b = vl.random_crop(vl.downsize(x), vl.downsize(x))
        assert a.shape == b.shape
        out[f"shape_{H}x{W}"] = np.array(a.shape[2:], np.int32)
    np.savez_compressed(OUT, **out)
    print("wrote", os.path.abspath(OUT), os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
