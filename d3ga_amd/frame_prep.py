"""Frame preparation: the image path of the reference's `Batcher.process` (lib/batch.py:150-163, 180, 205-208, 236) for a
whole batch in ONE HIP launch (csrc/frame_prep.hip) -- the foreground mask and its 7x7 median, `erode_mask`, `close_holes`,
`calibrate_color` (with `use_gamma_space`: `linear2color_corr`), the background fill and `get_silhouette`.

kornia is not vendored with the reference: its `median_blur` (zero padding, the 25th smallest of 49), `dilation` and `erosion`
(flat kernel, geodesic border: the in-image part of the window) are restated here from their documentation and stay unpinned
(DESIGN.md sec. 2).  GPU tensors only, no gradient; capturable (graph.CapturedStep) -- with `out=` the kernel writes straight
into a captured step's static target slots.
"""
import torch

from . import _lib
from ._lib import check, dptr, require_cuda, stream_handle

RED, GREEN, BLUE, GRAY = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.5, 0.5, 0.5)     # lib/batch.py:35-38
OUTPUTS = {"image": 3, "orig_image": 3, "alpha": 1, "silhouette": 3}                            # name -> channels


def _get(obj, key, default=None):
    """obj[key] / obj.key of a dict, an OmegaConf node or a plain object."""
    if isinstance(obj, dict):
        return obj.get(key, default)
    if hasattr(obj, "get") and callable(obj.get):
        try:
            return obj.get(key, default)
        except TypeError:
            pass
    return getattr(obj, key, default)


def _labels(cages, name):
    if name not in cages:
        return []
    ids = _get(cages[name], "label_id", None)
    if ids is None:
        raise ValueError(f"silhouette_table: cage {name!r} has no label_id")
    out = []
    for l in ids:
        l = int(l)
        if l == -1:                                          # get_mask skips it (lib/batch.py:114)
            continue
        if l <= 0:
            raise ValueError(f"silhouette_table: label {l} of cage {name!r}: the background label and negative labels other than -1 "
                             "cannot be painted (label 0 is always the background colour here)")
        out.append(l)
    return out


def silhouette_table(cages, background="white", device=None):
    """`Batcher.get_silhouette` (lib/batch.py:106-135) as a colour table: (label_rgb (n_labels,3) float32, other_rgb (3,)
    float32, bg_value).  Label 0 is the background (bg_value in all channels; row 0 of the table is not read); the labels of
    `upper` are red, then those of `lower` green, then those of `face` gray -- the reference paints in this order, so a label
    that sits in two lists takes the later colour; -1 is skipped; every other non-zero label is blue (other_rgb).  With the cages
    {body} or {body, face} the reference paints nothing red, green or gray: the face labels keep the background colour and
    everything else is blue.  cages: a dict-like of objects or dicts with `label_id`."""
    keys = list(cages.keys())
    bg = 1.0 if str(background).lower() == "white" else 0.0
    body_only = "body" in keys and (len(keys) == 1 or ("face" in keys and len(keys) == 2))
    if body_only:
        paint = [(_labels(cages, "face"), (bg, bg, bg))]
    else:
        paint = [(_labels(cages, "upper"), RED), (_labels(cages, "lower"), GREEN), (_labels(cages, "face"), GRAY)]
    n_labels = 1 + max([l for ids, _ in paint for l in ids], default=0)
    table = torch.tensor([BLUE], dtype=torch.float32).repeat(n_labels, 1)
    table[0] = bg
    for ids, rgb in paint:                                   # in the reference's order: later wins
        for l in ids:
            table[l] = torch.tensor(rgb)
    other = torch.tensor(BLUE, dtype=torch.float32)
    if device is not None:
        table, other = table.to(device), other.to(device)
    return table, other, bg


def _check_tensor(t, name, shape, dtypes, device=None):
    if not torch.is_tensor(t):
        raise ValueError(f"prepare_frames: {name} must be a tensor, got {type(t).__name__}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"prepare_frames: expected {name} {tuple(shape)}, got {tuple(t.shape)}")
    if t.dtype not in dtypes:
        raise ValueError(f"prepare_frames: {name} must be {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"prepare_frames: {name} must be contiguous")
    if device is not None and t.device != device:
        raise ValueError(f"prepare_frames: {name} is on {t.device}, the image on {device}")
    if t.data_ptr() % 16:
        raise ValueError(f"prepare_frames: {name} must be 16-byte aligned (a view with a storage offset? clone it)")


def prepare_frames(image, seg_part, seg_fg=None, *, table, gamma, background="white", erode_mask=False, close_holes=False, out=None):
    """The frame entries `image`, `orig_image`, `alpha` and `silhouette` of lib/batch.py:210-237 for B frames in one launch.
    image (B,3,H,W) float32 or uint8 (values 0..255, as the loader delivers them: a uint8 upload is a quarter the size);
    seg_part (B,1,H,W) int32, or float32 (truncated as `.int()` does); seg_fg (B,1,H,W) float32 or None (zeros);
    table: `silhouette_table(...)` with its tensors on the image's device; gamma: `train.use_gamma_space`.
    out: a dict with caller-owned float32 tensors under any of those four names -- written in place, nothing is allocated for
    them.  Returns a dict of (B,3|3|1|3,H,W) tensors plus `seg_fg`, the input passed through as it came (the reference's
    frames carry no binarised copy of it).  A shape, dtype, device, alignment or contiguity that does not fit raises ValueError;
    nothing is converted or copied behind the caller's back.  No gradient."""
    if not torch.is_tensor(image) or image.dim() != 4 or image.shape[1] != 3:
        raise ValueError(f"prepare_frames: expected image (B,3,H,W), got {tuple(image.shape) if torch.is_tensor(image) else type(image).__name__}")
    B, _, H, W = image.shape
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"prepare_frames: empty image {tuple(image.shape)}")
    dev = image.device
    _check_tensor(image, "image", (B, 3, H, W), (torch.float32, torch.uint8))
    _check_tensor(seg_part, "seg_part", (B, 1, H, W), (torch.int32, torch.float32), dev)
    if seg_fg is not None:
        _check_tensor(seg_fg, "seg_fg", (B, 1, H, W), (torch.float32,), dev)
    try:
        label_rgb, other_rgb, bg = table
    except (TypeError, ValueError):
        raise ValueError("prepare_frames: table must be the (label_rgb, other_rgb, bg_value) of silhouette_table") from None
    if not torch.is_tensor(label_rgb) or label_rgb.dim() != 2 or label_rgb.shape[0] < 1:
        raise ValueError("prepare_frames: table[0] must be a (n_labels,3) tensor")
    _check_tensor(label_rgb, "table[0]", (label_rgb.shape[0], 3), (torch.float32,), dev)
    _check_tensor(other_rgb, "table[1]", (3,), (torch.float32,), dev)
    if float(bg) != (1.0 if str(background).lower() == "white" else 0.0):
        raise ValueError(f"prepare_frames: the table was built for another background than {background!r}")
    out = dict(out or {})
    for name in out:
        if name not in OUTPUTS:
            raise ValueError(f"prepare_frames: out has no slot {name!r} (known: {', '.join(OUTPUTS)})")
        _check_tensor(out[name], f"out[{name!r}]", (B, OUTPUTS[name], H, W), (torch.float32,), dev)
    require_cuda(image)
    flags = (_lib.FRAME_GAMMA if gamma else 0) | (_lib.FRAME_BG_WHITE if bg else 0) | (_lib.FRAME_ERODE_MASK if erode_mask else 0) | \
            (_lib.FRAME_CLOSE_HOLES if close_holes else 0) | (_lib.FRAME_IMAGE_U8 if image.dtype == torch.uint8 else 0) | \
            (_lib.FRAME_SEG_F32 if seg_part.dtype == torch.float32 else 0)
    with torch.no_grad():
        for name, ch in OUTPUTS.items():
            if name not in out:
                out[name] = torch.empty(B, ch, H, W, dtype=torch.float32, device=dev)
        check(_lib.lib().d3ga_frame_prep(B, H, W, flags, dptr(image), dptr(seg_part), dptr(seg_fg), dptr(label_rgb), label_rgb.shape[0],
                                         dptr(other_rgb), dptr(out["image"]), dptr(out["orig_image"]), dptr(out["alpha"]),
                                         dptr(out["silhouette"]), stream_handle()), "d3ga_frame_prep")
    out["seg_fg"] = seg_fg
    return out


class FramePrep:
    """The image path of `Batcher` from the same configuration keys as `Batcher.__init__` (lib/batch.py:50-58):
    train.erode_mask, train.use_close_holes, train.use_gamma_space, train.background (default white) and `cages`.
    `prep(image, seg_part, seg_fg, out=None)` is the `prepare_frames` call; the colour table is built once and uploaded once per
    device."""

    def __init__(self, config):
        train = _get(config, "train")
        self.erode_mask = bool(_get(train, "erode_mask", False))
        self.close_holes = bool(_get(train, "use_close_holes", False))
        self.gamma = bool(_get(train, "use_gamma_space", False))
        bg = _get(train, "background", None)
        self.background = "white" if bg is None else str(bg).lower()
        self._table = silhouette_table(_get(config, "cages"), self.background)
        self._on_device = {}

    def table(self, device):
        key = str(device)
        if key not in self._on_device:
            self._on_device[key] = (self._table[0].to(device), self._table[1].to(device), self._table[2])
        return self._on_device[key]

    def __call__(self, image, seg_part, seg_fg=None, out=None):
        return prepare_frames(image, seg_part, seg_fg, table=self.table(image.device), gamma=self.gamma, background=self.background,
                              erode_mask=self.erode_mask, close_holes=self.close_holes, out=out)
