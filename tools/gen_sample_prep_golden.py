#!/usr/bin/env python3
"""Generate tests/golden/sample_prep_cases.npz -- and nothing else -- by running the reference's OWN loader lines on the CPU:
datasets.actorshq_dataset.ActorsHQDataset.get_boundary_mask and ActorsHQDataset.__getitem__ (an unbound dataset: object.__new__
plus the attributes __getitem__ reads).

Runs only where the reference checkout is present.  The import-stub harness is tools/gen_golden.py's `install_harness`; cv2 is
one of its stubs, and three of its functions are given a meaning here:
    cv2.imread   served from the arrays of the case, by the path's prefix (image / seg / alpha)
    cv2.erode, cv2.dilate   scipy.ndimage.minimum_filter / maximum_filter over the kernel's footprint with the border filled by
                 the neutral value (255 / 0) -- the border-ignoring behaviour of cv2's default border value, restated.  This
                 stand-in is the one part of the recorded results that the reference does not hold: parity with cv2 is unpinned.

Arrays only.  Three cases: a 40 x 48 frame with a part image larger by (2, 5); a 37 x 45 one of equal size; a 41 x 47 one whose
matte is mostly soft values.  Every case holds the matte values 0, 5, 6, 127, 128, 129, 249, 250, 255, part colours of every
branch of the label rule, black and a native red of 127.  Recorded per case: the inputs, `seg_part`, `seg_fg`, `boundary_fg` and
`image` of the sample, and get_boundary_mask's two results called on its own."""
import os
import sys

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as gg  # noqa: E402

OUT = os.path.join(HERE, "..", "tests", "golden", "sample_prep_cases.npz")
CASES = {"a": (40, 48, (2, 5), 0.3), "b": (37, 45, (0, 0), 0.3), "c": (41, 47, (1, 0), 0.8)}


def make_case(seed, H, W, extra, soft):
    rng = np.random.default_rng(seed)
    image = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    coarse = rng.random((H // 5 + 1, W // 5 + 1)) < 0.5
    alpha = np.where(np.kron(coarse, np.ones((5, 5), bool))[:H, :W], 255, 0).astype(np.uint8)
    special = np.array([0, 5, 6, 127, 128, 129, 249, 250, 255, 128, 1, 64, 200], np.uint8)
    pick = rng.random((H, W)) < soft
    alpha[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    alpha.reshape(-1)[:9] = special[:9]
    alpha3 = np.stack([alpha, rng.integers(0, 256, (H, W), dtype=np.uint8), alpha], axis=-1)       # only channel 0 is the matte
    palette = np.array([[0, 0, 255], [0, 255, 0], [255, 0, 0], [127, 127, 127], [0, 0, 0], [9, 200, 127], [255, 255, 255], [255, 0, 127],
                        [0, 255, 255], [3, 4, 5], [127, 255, 255]], np.uint8)                      # BGR
    seg = palette[rng.integers(0, len(palette), (H + extra[0], W + extra[1]))]
    noise = rng.random(seg.shape[:2]) < 0.1
    seg[noise] = rng.integers(0, 256, (int(noise.sum()), 3), dtype=np.uint8)
    return image, seg, alpha3


def main():
    gg.install_harness()
    import cv2
    import datasets.actorshq_dataset as mod

    files = {}
    cv2.imread = lambda path, *a: files[os.path.basename(path).split("_")[0]].copy()
    foot = lambda kernel: np.asarray(kernel) != 0
    cv2.erode = lambda src, kernel: ndimage.minimum_filter(src, footprint=foot(kernel), mode="constant", cval=255)
    cv2.dilate = lambda src, kernel: ndimage.maximum_filter(src, footprint=foot(kernel), mode="constant", cval=0)
    real_exists = os.path.exists
    os.path.exists = lambda p: True if str(p).startswith("seg_") else real_exists(p)

    ds = object.__new__(mod.ActorsHQDataset)
    ds.warmup, ds.eval, ds.internal_counter = False, True, 0
    ds.frame_list = [["Sequence1", "000007"]]
    ds.test_camera = ["Cam001"]
    ds.cameras = {"Cam001": {"K": np.eye(3, dtype=np.float32)}}
    ds.cam2idx = {"Cam001": 0}
    ds.smplx = {"Sequence1": {7: {"poses": np.zeros(165, np.float32)}}}
    ds.image_path, ds.image_part_mask_path, ds.image_alpha = "image_{frame:06d}.png", "seg_{frame:06d}.png", "alpha_{frame:06d}.png"

    out = {"names": np.array(list(CASES))}
    for i, (name, (H, W, extra, soft)) in enumerate(CASES.items()):
        image, seg, alpha3 = make_case(90 + i, H, W, extra, soft)
        files.update(image=image, seg=seg, alpha=alpha3)
        sample = ds[0]
        boundary, fg = mod.ActorsHQDataset.get_boundary_mask(alpha3[:, :, 0].copy())
        assert sample["image"].shape == (3, H, W) and sample["image"].dtype == np.float32
        assert sample["seg_part"].shape == (1, H, W) and sample["seg_part"].dtype == np.int32
        assert sample["seg_fg"].dtype == np.bool_ and sample["boundary_fg"].dtype == np.bool_
        assert np.array_equal(sample["seg_fg"][0], fg) and np.array_equal(sample["boundary_fg"][0], boundary)
        assert set(np.unique(sample["seg_part"]).tolist()) == {0, 1, 2, 3, 4} and (alpha3[:, :, 0] == 128).sum() > 3
        out.update({f"{name}_image_bgr": image, f"{name}_seg_bgr": seg, f"{name}_alpha_bgr": alpha3,
                    f"{name}_image": sample["image"], f"{name}_seg_part": sample["seg_part"], f"{name}_seg_fg": sample["seg_fg"],
                    f"{name}_boundary_fg": sample["boundary_fg"], f"{name}_mask_boundary": boundary, f"{name}_mask_fg": fg})
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT))


if __name__ == "__main__":
    main()
