"""Sample preparation (csrc/sample_prep.hip): the numpy lines of the loader workers between the decoded files and
the tensors of a sample, for a whole batch in ONE HIP launch.

    datasets/actorshq_dataset.py:244-276 (get_boundary_mask :201-217)      prepare_actorshq(image_bgr, seg_bgr, mask)
    datasets/goliath_dataset.py:454-481 (the halving F.interpolate calls)   prepare_goliath(image, parts)

A worker returns the uint8 arrays as the decoder delivers them -- 7 bytes per pixel over the bus instead of 18 -- and the launch
writes what `prepare_frames`, `compose_target` and the `Evaluator` take: `image` (planar RGB), `seg_part`, `seg_fg`, `boundary_fg`.
`SamplePrep(config)` chains the launch with `FramePrep`: the pixel-dependent frame entries of lib/batch.py:210-237 in two launches.

The rules are pinned by csrc/sample_prep_math.h, whose g++ build gives the kernels' bytes.  cv2's erode / dilate border and anchor
are restated from their documentation and stay unpinned; torch's own uint8 bilinear resize (a rounded fixed-point result) is
deliberately not reproduced: the Goliath outputs are `F.interpolate` of the FLOAT image, bit for bit.  GPU tensors only, no
gradient, no synchronisation; capturable.  Strided inputs are taken as they are -- nothing is converted or copied behind the
caller's back, and what cannot be addressed raises ValueError."""
import torch

from . import _lib
from ._lib import check, dptr, require_cuda, stream_handle
from .frame_prep import FramePrep

OUTPUTS = {"image": 3, "seg_part": 1, "seg_fg": 1, "boundary_fg": 1}                            # name -> channels
FRAME_OUTPUTS = ("image", "orig_image", "alpha", "silhouette", "boundary_fg", "seg_fg", "seg_part")


def _u8_source(t, name, fn, tail):
    """A uint8 tensor (B, H, W) + tail, tail being the trailing dimensions that must be dense (e.g. (3,) for interleaved pixels).
    Strides of dimensions of size 1 carry no information and are not looked at."""
    if t.dtype != torch.uint8:
        raise ValueError(f"{fn}: {name} must be uint8, got {t.dtype}")
    dense = 1
    for size, stride in zip(reversed(tail), reversed(t.stride()[3:])):
        if size > 1 and stride != dense:
            raise ValueError(f"{fn}: {name} has strides {t.stride()}: the {tail} at the end must be dense")
        dense *= size


def _rows(t, name, fn, step, row_bytes):
    """(pitch, frame) of a (B, H, W, ...) uint8 view whose pixels are `step` bytes apart and whose rows span row_bytes"""
    B, H, W = t.shape[:3]
    sb, sh, sw = t.stride()[:3]
    if W > 1 and sw != step:
        raise ValueError(f"{fn}: {name} has strides {t.stride()}: pixels must be {step} byte(s) apart")
    pitch = sh if H > 1 else row_bytes
    if pitch < row_bytes:
        raise ValueError(f"{fn}: {name} has strides {t.stride()}: a row pitch of {pitch} bytes is smaller than the row ({row_bytes})")
    frame = sb if B > 1 else 0
    if B > 1 and frame < (H - 1) * pitch + row_bytes:
        raise ValueError(f"{fn}: {name} has strides {t.stride()}: frames overlap (a frame spans {(H - 1) * pitch + row_bytes} bytes)")
    return pitch, frame


def _outputs(fn, out, names, shapes, dtypes, dev):
    """Validate the caller's slots and allocate the rest"""
    out = dict(out or {})
    for name in out:
        if name not in names:
            raise ValueError(f"{fn}: out has no slot {name!r} (known: {', '.join(names)})")
        t = out[name]
        if not torch.is_tensor(t):
            raise ValueError(f"{fn}: out[{name!r}] must be a tensor, got {type(t).__name__}")
        if tuple(t.shape) != shapes[name]:
            raise ValueError(f"{fn}: expected out[{name!r}] {shapes[name]}, got {tuple(t.shape)}")
        if t.dtype not in dtypes[name]:
            raise ValueError(f"{fn}: out[{name!r}] must be {' or '.join(str(d) for d in dtypes[name])}, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{fn}: out[{name!r}] must be contiguous")
        if t.device != dev:
            raise ValueError(f"{fn}: out[{name!r}] is on {t.device}, the inputs on {dev}")
        if t.dtype != torch.uint8 and t.data_ptr() % 16:
            raise ValueError(f"{fn}: out[{name!r}] must be 16-byte aligned (a view with a storage offset? clone it)")
    return out


def prepare_actorshq(image_bgr, seg_bgr, mask, *, image_dtype=torch.uint8, out=None):
    """The ActorsHQ sample from the three decoded arrays, B frames in one launch.
    image_bgr (B,H,W,3), seg_bgr (B,Hs,Ws,3) with Hs >= H and Ws >= W (its top-left H x W is read), mask (B,H,W) or (B,H,W,3)
    (channel 0 is the matte): uint8 tensors on the GPU; without the leading B for a single frame.  Row pitches, frame strides and
    the mask's pixel step (1 or 3) come from the tensors' strides: crops `x[:, :h, :w]`, row-padded buffers and the channel view
    `matte[..., 0]` are addressed in place.
    image_dtype: torch.uint8 or torch.float32 for the allocated `image` (a slot in `out` decides for itself).
    out: a dict with caller-owned tensors under any of `image` (B,3,H,W) uint8 or float32, `seg_part` (B,1,H,W) int32, `seg_fg`,
    `boundary_fg` (B,1,H,W) float32 -- written in place, nothing is allocated for them.  Returns the dict of all four."""
    fn = "prepare_actorshq"
    if not torch.is_tensor(image_bgr) or image_bgr.dim() not in (3, 4) or image_bgr.shape[-1] != 3:
        raise ValueError(f"{fn}: expected image_bgr (B,H,W,3) or (H,W,3), got "
                         f"{tuple(image_bgr.shape) if torch.is_tensor(image_bgr) else type(image_bgr).__name__}")
    single = image_bgr.dim() == 3
    for name, t in (("seg_bgr", seg_bgr), ("mask", mask)):
        if not torch.is_tensor(t):
            raise ValueError(f"{fn}: {name} must be a tensor, got {type(t).__name__}")
    if single:
        image_bgr, seg_bgr, mask = image_bgr[None], seg_bgr[None], mask[None]
    B, H, W, _ = image_bgr.shape
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"{fn}: empty image {tuple(image_bgr.shape)}")
    if seg_bgr.dim() != 4 or seg_bgr.shape[0] != B or seg_bgr.shape[3] != 3 or seg_bgr.shape[1] < H or seg_bgr.shape[2] < W:
        raise ValueError(f"{fn}: expected seg_bgr (B,Hs,Ws,3) with B = {B}, Hs >= {H}, Ws >= {W}, got {tuple(seg_bgr.shape)}")
    Hs, Ws = seg_bgr.shape[1:3]
    if mask.dim() == 4 and mask.shape[3] == 3:
        mask = mask[..., 0]
    if tuple(mask.shape) != (B, H, W):
        raise ValueError(f"{fn}: expected mask {(B, H, W)} or {(B, H, W, 3)}, got {tuple(mask.shape)}")
    dev = image_bgr.device
    for name, t in (("seg_bgr", seg_bgr), ("mask", mask)):
        if t.device != dev:
            raise ValueError(f"{fn}: {name} is on {t.device}, the image on {dev}")
    _u8_source(image_bgr, "image_bgr", fn, (3,))
    _u8_source(seg_bgr, "seg_bgr", fn, (3,))
    _u8_source(mask, "mask", fn, ())
    image_pitch, image_frame = _rows(image_bgr, "image_bgr", fn, 3, 3 * W)
    seg_pitch, seg_frame = _rows(seg_bgr[:, :H], "seg_bgr", fn, 3, 3 * Ws)
    mask_step = mask.stride(2) if W > 1 else 1
    if mask_step not in (1, 3):
        raise ValueError(f"{fn}: mask has strides {mask.stride()}: its pixels must be 1 or 3 bytes apart (a plane, or channel 0 of (H,W,3))")
    mask_pitch, mask_frame = _rows(mask, "mask", fn, mask_step, (W - 1) * mask_step + 1)
    if image_dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"{fn}: image_dtype must be torch.uint8 or torch.float32, got {image_dtype}")
    shapes = {n: (B, c, H, W) for n, c in OUTPUTS.items()}
    dtypes = {"image": (torch.uint8, torch.float32), "seg_part": (torch.int32,), "seg_fg": (torch.float32,), "boundary_fg": (torch.float32,)}
    out = _outputs(fn, out, OUTPUTS, shapes, dtypes, dev)
    require_cuda(image_bgr, seg_bgr, mask)
    with torch.no_grad():
        for name in OUTPUTS:
            if name not in out:
                out[name] = torch.empty(shapes[name], dtype=image_dtype if name == "image" else dtypes[name][0], device=dev)
        check(_lib.lib().d3ga_sample_prep_actorshq(B, H, W, Hs, Ws, dptr(image_bgr), image_pitch, image_frame, dptr(seg_bgr), seg_pitch, seg_frame,
                                                   dptr(mask), mask_pitch, mask_frame, mask_step, int(out["image"].dtype == torch.float32),
                                                   dptr(out["image"]), dptr(out["seg_part"]), dptr(out["seg_fg"]), dptr(out["boundary_fg"]),
                                                   None, stream_handle()), "d3ga_sample_prep_actorshq")
    return out


def prepare_goliath(image, parts, *, out=None):
    """The Goliath sample at half size from the decoded uint8 tensors, B frames in one launch: `F.interpolate(x.float(),
    scale_factor=0.5, mode="bilinear")` of the image, of the part labels and of (parts != 0), bit for bit, and boundary_fg =
    1 - seg_fg.  image (B,3,H,W), parts (B,1,H,W) uint8 on the GPU (without B for a single frame), H, W >= 2, elements of a row
    dense; row pitches, plane and frame strides come from the tensors.  Returns / writes (out=) float32 `image` (B,3,H//2,W//2) and
    `seg_part`, `seg_fg`, `boundary_fg` (B,1,H//2,W//2); `prepare_frames` truncates seg_part as `.int()` does."""
    fn = "prepare_goliath"
    if not torch.is_tensor(image) or image.dim() not in (3, 4) or image.shape[-3] != 3:
        raise ValueError(f"{fn}: expected image (B,3,H,W) or (3,H,W), got {tuple(image.shape) if torch.is_tensor(image) else type(image).__name__}")
    if not torch.is_tensor(parts):
        raise ValueError(f"{fn}: parts must be a tensor, got {type(parts).__name__}")
    if image.dim() == 3:
        image, parts = image[None], parts[None]
    B, _, H, W = image.shape
    if B < 1 or H < 2 or W < 2:
        raise ValueError(f"{fn}: image {tuple(image.shape)}: halving needs B >= 1 and H, W >= 2")
    if tuple(parts.shape) != (B, 1, H, W):
        raise ValueError(f"{fn}: expected parts {(B, 1, H, W)}, got {tuple(parts.shape)}")
    dev = image.device
    if parts.device != dev:
        raise ValueError(f"{fn}: parts is on {parts.device}, the image on {dev}")
    for name, t in (("image", image), ("parts", parts)):
        if t.dtype != torch.uint8:
            raise ValueError(f"{fn}: {name} must be uint8, got {t.dtype} (the float form is what this launch produces)")
    # (B, C, H, W) -> rows of (B C) "frames": the plane stride of the image must hold a plane, its frame stride three of them
    image_pitch, _ = _rows(image[:, 0], "image", fn, 1, W)
    parts_pitch, parts_frame = _rows(parts[:, 0], "parts", fn, 1, W)
    image_plane, image_frame = image.stride(1), (image.stride(0) if B > 1 else 0)
    span = (H - 1) * image_pitch + W
    if image_plane < span or (B > 1 and image_frame < 2 * image_plane + span):
        raise ValueError(f"{fn}: image has strides {image.stride()}: channels or frames overlap")
    oh, ow = H // 2, W // 2
    shapes = {n: (B, c, oh, ow) for n, c in OUTPUTS.items()}
    out = _outputs(fn, out, OUTPUTS, shapes, {n: (torch.float32,) for n in OUTPUTS}, dev)
    require_cuda(image, parts)
    with torch.no_grad():
        for name in OUTPUTS:
            if name not in out:
                out[name] = torch.empty(shapes[name], dtype=torch.float32, device=dev)
        check(_lib.lib().d3ga_sample_prep_goliath(B, H, W, dptr(image), image_pitch, image_plane, image_frame, dptr(parts), parts_pitch, parts_frame,
                                                  dptr(out["image"]), dptr(out["seg_part"]), dptr(out["seg_fg"]), dptr(out["boundary_fg"]),
                                                  None, stream_handle()), "d3ga_sample_prep_goliath")
    return out


class SamplePrep:
    """From the decoded arrays to the frame entries of lib/batch.py:210-237 that depend on pixels -- `image`, `orig_image`,
    `alpha`, `silhouette`, `boundary_fg`, `seg_fg` (and `seg_part`, the labels they were made from) -- in two launches: sample
    preparation, then the `FramePrep` this object owns (built from the same configuration keys as `Batcher`).
    out: a dict with caller-owned tensors under any of those names (float32; seg_part int32 in ActorsHQ mode), written in place --
    the static slots of a captured step."""

    def __init__(self, config):
        self.frame_prep = FramePrep(config)

    def _run(self, fn, sample, out):
        out = dict(out or {})
        for name in out:
            if name not in FRAME_OUTPUTS:
                raise ValueError(f"{fn}: out has no slot {name!r} (known: {', '.join(FRAME_OUTPUTS)})")
        s = sample({n: out[n] for n in ("seg_part", "seg_fg", "boundary_fg") if n in out})
        frames = self.frame_prep(s["image"], s["seg_part"], s["seg_fg"], out={n: out[n] for n in ("image", "orig_image", "alpha", "silhouette") if n in out})
        frames["boundary_fg"], frames["seg_part"] = s["boundary_fg"], s["seg_part"]
        return frames

    def actorshq(self, image_bgr, seg_bgr, mask, out=None):
        """The uint8 image goes from the first launch to the second as it is (a quarter of the float's bytes)."""
        return self._run("SamplePrep.actorshq", lambda slots: prepare_actorshq(image_bgr, seg_bgr, mask, out=slots), out)

    def goliath(self, image, parts, out=None):
        return self._run("SamplePrep.goliath", lambda slots: prepare_goliath(image, parts, out=slots), out)
