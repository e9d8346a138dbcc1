"""Float64 / boolean numpy oracle of frame preparation (d3ga_amd/frame_prep.py, csrc/frame_prep.hip): the image path of the
reference's Batcher.process (lib/batch.py:150-163, 180, 205-208, 236), restated operation by operation.

The median is taken literally -- the 49 values of the zero-padded 7x7 window are sorted and element 24 is returned -- and
dilation / erosion are the maximum / minimum over the part of the window that lies inside the image.  Nothing here counts, so
the kernel's majority-vote formulation is checked against an independent one.

Pinned by the reference itself (tests/golden/frame_cases.npz, tools/gen_golden.py: gen_frames): linear2color_corr and
Batcher.get_silhouette.  NOT pinned: the median and the morphology -- kornia is not vendored with the reference, their rules are
restated from its documentation (median_blur: zero padding; dilation / erosion with a flat kernel: geodesic border)."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

RED, GREEN, BLUE, GRAY = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.5, 0.5, 0.5)


def labels_ref(seg_part):
    """.int() of the label map: truncation toward zero."""
    return np.trunc(np.asarray(seg_part, dtype=np.float64)).astype(np.int64)


def fg_ref(seg_part, seg_fg=None):
    s = labels_ref(seg_part)
    return (s > 0) if seg_fg is None else ((s > 0) | (np.asarray(seg_fg) > 0))


def _windows(m, k, fill):
    """(..., H, W, k*k): the k x k window around every pixel of the last two axes, `fill` outside the image."""
    r = k // 2
    pad = [(0, 0)] * (m.ndim - 2) + [(r, r), (r, r)]
    p = np.pad(np.asarray(m, dtype=np.float64), pad, constant_values=fill)
    w = sliding_window_view(p, (k, k), axis=(-2, -1))
    return w.reshape(w.shape[:-2] + (k * k,))


def median_ref(m, k=7):
    return np.sort(_windows(m, k, 0.0), axis=-1)[..., (k * k) // 2]


def dilate_ref(m, k):
    return _windows(m, k, -np.inf).max(axis=-1)


def erode_ref(m, k):
    return _windows(m, k, np.inf).min(axis=-1)


def alpha_ref(fg, erode_mask=False, close_holes=False):
    a = median_ref(np.asarray(fg, dtype=np.float64), 7)
    if erode_mask:                                           # utils/image_utils.py:49-58
        a = erode_ref(dilate_ref(a, 7), 5)
    if close_holes:                                          # :61-70
        a = erode_ref(dilate_ref(a, 5), 5)
    return a


def linear2color_ref(img, dim):
    """utils/image_utils.py:92-113 in float64; the three channels along `dim`.  The reference holds the channel scales in a
    FloatTensor, so they are the float32 roundings of 1.4, 1.1 and 1.6 whatever the image's precision."""
    img = np.asarray(img, dtype=np.float64)
    black = 3.0 / 255.0
    scale = np.array([1.4, 1.1, 1.6], dtype=np.float32).astype(np.float64).reshape([3 if i == dim % img.ndim else 1 for i in range(img.ndim)])
    x = img * scale / 1.1
    return np.clip(np.sqrt((1.0 / (1.0 - black)) * 0.95 * np.clip(x - black, 0.0, 2.0)) - 15.0 / 255.0, 0.0, 2.0)


def orig_ref(image, gamma):
    """calibrate_color (lib/batch.py:78-88) without a CCM; image (B,3,H,W), values 0..255."""
    x = np.asarray(image, dtype=np.float64) / 255.0
    return linear2color_ref(x, 1) if gamma else x


def _label_ids(cages, name):
    if name not in cages:
        return [-1]
    c = cages[name]
    return list(c["label_id"] if isinstance(c, dict) else c.label_id)


def silhouette_ref(seg_part, cages, background):
    """get_silhouette (lib/batch.py:106-135) with masks, as the reference does it; seg_part (H,W) integers -> (3,H,W)."""
    s = np.asarray(seg_part)
    sil = np.ones(s.shape + (3,)) * float(background == "white")

    def mask(labels):
        m = np.zeros(s.shape, dtype=bool)
        for l in labels:
            if l != -1:
                m |= s == l
        return m

    keys = list(cages.keys())
    if ("body" in keys and len(keys) == 1) or ("body" in keys and "face" in keys and len(keys) == 2):
        body = ~(s == 0) & ~mask(_label_ids(cages, "face"))
    else:
        upper, lower, face = (mask(_label_ids(cages, n)) for n in ("upper", "lower", "face"))
        body = ~(s == 0) & ~upper & ~lower & ~face
        sil[upper] = RED
        sil[lower] = GREEN
        sil[face] = GRAY
    sil[body] = BLUE
    return np.moveaxis(sil, -1, 0)


def frame_ref(image, seg_part, seg_fg, cages, gamma, background="white", erode_mask=False, close_holes=False):
    """image (B,3,H,W), seg_part / seg_fg (B,1,H,W) -> dict of float64 arrays, `fg` boolean."""
    fg = fg_ref(seg_part, seg_fg)
    orig = orig_ref(image, gamma)
    f = fg.astype(np.float64)
    img = orig * f + (1.0 - f) if background == "white" else orig * f
    s = labels_ref(seg_part)
    sil = np.stack([silhouette_ref(s[b, 0], cages, background) for b in range(s.shape[0])])
    return {"fg": fg, "orig_image": orig, "image": img, "alpha": alpha_ref(f, erode_mask, close_holes), "silhouette": sil}
