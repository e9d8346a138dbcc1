"""PNG files of the recorder's written images (csrc/png.hip): a uint8 image on the GPU becomes the bytes of its PNG
file in two launches, so that what crosses the bus is the finished file and the save pool only calls write().

Drop-ins for
    test.py:182-195     torchvision.utils.save_image(img, path)                      save_image(img, path)
    train.py:365-371    cv2.imwrite(path, np.clip(grid * 255, 0, 255)) in BGR        encode_png(compose_grid(rows, quantize="clip", order="rgb"))

    buf = PngBuffer(H, W, 3)                          # once per image size: the file's bytes and the scratch, one allocation
    encode_png(grid_u8, out=buf)                      # two launches, no synchronisation, capturable with out=
    handle = writer.submit_png(buf)                   # one asynchronous copy; handle.save(path) in the save pool's thread

The byte stream -- strips, filters, run tokens, tables, checksums -- is pinned by csrc/png_math.h, whose g++ build gives the same
bytes as the kernels.  There is no CPU path: host arrays are refused.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, stream_handle

__all__ = ["PngBuffer", "encode_png", "png_bytes", "save_image", "FILTERS"]

FILTERS = {"adaptive": _lib.PNG_FILTER_ADAPTIVE, 0: 0, 1: 1, 2: 2, 3: 3, 4: 4}
_INT32_MAX = 2 ** 31 - 1


def _sizes(H, W, C, rows_per_strip, what):
    """(capacity, scratch bytes) of an image, or the ValueError / TypeError that names the argument.  Touches no device."""
    for name, v in (("H", H), ("W", W), ("C", C), ("rows_per_strip", rows_per_strip)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"{what}: {name} must be an integer, got {type(v).__name__}")
    if C not in (1, 3, 4):
        raise ValueError(f"{what}: C={C} channels, expected 1, 3 or 4")
    if H < 1 or H > _INT32_MAX:
        raise ValueError(f"{what}: H={H}, expected 1..{_INT32_MAX}")
    if W < 1 or W > _INT32_MAX // C:
        raise ValueError(f"{what}: W={W}, expected 1..{_INT32_MAX // C} with C={C}")
    if rows_per_strip < 0 or rows_per_strip > _INT32_MAX:
        raise ValueError(f"{what}: rows_per_strip={rows_per_strip}, expected 0 (the default) or a positive number of rows")
    scratch = ctypes.c_int64(0)
    cap = _lib.lib().d3ga_png_capacity(int(H), int(W), int(C), int(rows_per_strip), ctypes.byref(scratch))
    if cap < 0:
        raise ValueError(f"{what}: rows_per_strip={rows_per_strip} rows of W={W} x C={C} exceed a strip's {_INT32_MAX} filtered bytes")
    return int(cap), int(scratch.value)


class PngBuffer:
    """The bytes of one PNG file on the device, reusable across calls: ONE allocation laid out as
    [uint64 length][PNG bytes up to .capacity][scratch].  .buffer is the view [length word | PNG bytes] -- what
    GridWriter.submit_png copies -- and .shape the (H, W, C) it was sized for."""

    def __init__(self, H, W, C, rows_per_strip=0, device=None):
        self.capacity, self.scratch_bytes = _sizes(H, W, C, rows_per_strip, "PngBuffer")
        self.shape, self.rows_per_strip = (int(H), int(W), int(C)), int(rows_per_strip)
        head = (16 + self.capacity + 15) & ~15               # 8 spare bytes in front: the PNG bytes and the scratch start 16-byte aligned
        self.storage = torch.empty(head + self.scratch_bytes, dtype=torch.uint8, device="cuda" if device is None else device)
        if not self.storage.is_cuda:
            raise ValueError(f"PngBuffer: device={device!r}; the encoder runs on the GPU only")
        self.buffer = self.storage[8:16 + self.capacity]
        self.scratch = self.storage[head:]

    def __repr__(self):
        return f"PngBuffer({self.shape[0]}x{self.shape[1]}x{self.shape[2]}, capacity {self.capacity})"


def _check_image(img):
    if not torch.is_tensor(img):
        raise TypeError(f"encode_png: img_u8 must be a uint8 tensor on the GPU, got {type(img).__name__}; host arrays have no path "
                        "in this library")
    if img.dtype != torch.uint8:
        raise TypeError(f"encode_png: img_u8 must be uint8, got {img.dtype} (to_uint8 converts a float image)")
    if not img.is_cuda:
        raise ValueError(f"encode_png: img_u8 is on {img.device}; the encoder runs on the GPU only")
    if img.dim() != 3:
        raise ValueError(f"encode_png: img_u8 must be (H, W, C), got {tuple(img.shape)}")
    H, W, C = (int(v) for v in img.shape)
    if C not in (1, 3, 4):
        raise ValueError(f"encode_png: img_u8 has C={C} channels, expected 1, 3 or 4")
    if H < 1 or W < 1:
        raise ValueError(f"encode_png: img_u8 is empty, H={H} W={W}")
    sh, sw, sc = img.stride()
    if sc != 1 or sw != C or (H > 1 and sh < W * C):
        raise ValueError(f"encode_png: img_u8 has strides {img.stride()}: pixels must be dense, rows may be padded")
    return H, W, C, int(sh) if H > 1 else W * C


def encode_png(img_u8, *, filter="adaptive", rows_per_strip=0, out=None):
    """img_u8: uint8 (H, W, C) on the GPU, C in {1, 3, 4} (grey, RGB, RGBA), unit inner strides, rows at least W C apart.
    filter: "adaptive" (per row the type with the smallest sum of absolute values) or 0..4 to force None, Sub, Up, Average,
    Paeth.  rows_per_strip: rows per independently compressed strip; 0 takes `out`'s, else the default for (H, W, C).
    Returns the PngBuffer that holds the file (png_bytes reads it back; GridWriter.submit_png copies it asynchronously).

    Two launches, no synchronisation; with out= no allocation either, so the call can sit in a captured graph.  Anything the
    encoder does not take raises TypeError / ValueError naming the argument before a launch."""
    H, W, C, pitch = _check_image(img_u8)
    if filter not in FILTERS or isinstance(filter, bool):
        raise ValueError(f"encode_png: filter={filter!r}, expected 'adaptive' or 0..4")
    if out is not None and not isinstance(out, PngBuffer):
        raise TypeError(f"encode_png: out must be a PngBuffer, got {type(out).__name__}")
    rows = rows_per_strip if (rows_per_strip or out is None) else out.rows_per_strip
    capacity, scratch_bytes = _sizes(H, W, C, rows, "encode_png")
    _lib.require_cuda(img_u8)
    if out is None:
        out = PngBuffer(H, W, C, rows, device=img_u8.device)
    else:
        if out.capacity < capacity or out.scratch_bytes < scratch_bytes:
            raise ValueError(f"encode_png: out is too small: {out!r} with {out.scratch_bytes} bytes of scratch, an image "
                             f"{H}x{W}x{C} at rows_per_strip={rows} needs {capacity} and {scratch_bytes}")
        _lib.require_cuda(out.storage)
    args = (H, W, C, pitch, FILTERS[filter], int(rows), img_u8.data_ptr(), out.buffer.data_ptr(), out.capacity, out.scratch.data_ptr(),
            out.scratch_bytes)
    L = _lib.lib()
    st = L.d3ga_png_check(*args)
    if st != 0:
        raise ValueError(f"encode_png: refused with status {st} ({L.d3ga_status_string(st).decode()}) for img_u8 {H}x{W}x{C}, "
                         f"pitch {pitch}, rows_per_strip={rows}")
    check(L.d3ga_png_encode(*args, stream_handle()), "d3ga_png_encode")
    out.encoded_shape = (H, W, C)
    return out


def png_bytes(buf):
    """The file's bytes: ONE synchronising read-back of the whole buffer (tests and small use; the frame loop uses
    GridWriter.submit_png)."""
    if not isinstance(buf, PngBuffer):
        raise TypeError(f"png_bytes: expected a PngBuffer, got {type(buf).__name__}")
    host = buf.buffer.cpu().numpy()
    n = int(host[:8].view(np.uint64)[0])
    if n > buf.capacity:
        raise _lib.D3GAError(f"png_bytes: the length word says {n} bytes, the buffer holds {buf.capacity}: nothing was encoded into it")
    return host[8:8 + n].tobytes()


def save_image(tensor, path):
    """torchvision.utils.save_image for ONE image, without torchvision or PIL: a float32 (C, H, W) image goes through to_uint8
    (save_image's own rounding; one channel is written as grey-valued RGB, as make_grid does), a uint8 (H, W, C) image is
    written as it is.  A blocking write."""
    if not torch.is_tensor(tensor):
        raise TypeError(f"save_image: tensor must be a tensor on the GPU, got {type(tensor).__name__}")
    if tensor.dtype != torch.uint8:
        from .frame_grid import to_uint8
        tensor = to_uint8(tensor)
    data = png_bytes(encode_png(tensor))
    with open(path, "wb") as f:
        f.write(data)
