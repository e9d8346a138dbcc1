"""The recorder's frame grid (csrc/frame_grid.hip): labels, panels, padding and the uint8 conversion of a
written image as ONE launch, with the label font of csrc/frame_grid_font.h and no read-back.

Drop-ins for
    utils/text_helpers.py:27-50   write_text(img, text, fontColor, thickness, bottom, X)     write_text(...) on device tensors
    test.py:145-179               th.cat rows, th.cat grid, F.pad to even sizes              compose_grid(rows, pad_even=True)
    test.py:182-195               torchvision.utils.save_image's float -> uint8              quantize="save_image", to_uint8(img)
    train.py:344-365              the 2 x 5 progress grid, np.clip(grid * 255) in BGR        quantize="clip", order="bgr"
    test.py:156, train.py:347     f"{psnr:.3f} (dB)"                                          Panel(..., label="{:.3f} (dB)", value=cell)

    rows = [[Panel(pred, "Prediction"), Panel(mesh, "Input: Cage"), Panel(pts, "Input: Points")],
            [Panel(means, "3D Means"), Panel(normals, "Output: Normals"), Panel(heat, "{:.3f} (dB)", color=(1, 1, 1), value=ev.psnr_cell)]]
    grid = compose_grid(rows, out=grid_u8)            # (H, W, 3) uint8, one launch, capturable with out=
    handle = writer.submit(grid)                      # one asynchronous copy; handle.numpy() in the save pool's thread

There is no CPU path: host arrays are refused.  Glyph shapes are the project's own (parity with cv2's Hershey strokes is
unpinned); everything else -- layout rule, coverage, blend, both quantisers, the number format -- is pinned bit for bit to the
g++ build of csrc/frame_grid_math.h.
"""
import ctypes
import threading

import numpy as np
import torch

from . import _lib
from ._lib import check, stream_handle

__all__ = ["Panel", "compose_grid", "compose_panels", "to_uint8", "write_text", "GridWriter", "MAX_PANELS", "MAX_LABEL"]

MAX_PANELS = _lib.GRID_MAX_PANELS
MAX_LABEL = _lib.GRID_MAX_LABEL
SLOT = "{:.3f}"
_MODES = {None: None, "save_image": _lib.GRID_OUT_U8_SAVE_IMAGE, "clip": _lib.GRID_OUT_U8_CLIP}


def _geometry(img, layout, what):
    """(C, h, w, sc, sh, sw) of a (C,H,W) | (H,W,C) | (H,W) tensor: sizes and ELEMENT strides, whatever view it is."""
    if layout not in ("chw", "hwc"):
        raise ValueError(f"{what}: layout {layout!r}, expected 'chw' or 'hwc'")
    if img.dim() == 2:
        (h, w), (sh, sw) = img.shape, img.stride()
        c, sc = 1, 0
    elif img.dim() == 3 and layout == "chw":
        (c, h, w), (sc, sh, sw) = img.shape, img.stride()
    elif img.dim() == 3:
        (h, w, c), (sh, sw, sc) = img.shape, img.stride()
    else:
        raise ValueError(f"{what}: expected an image (C,H,W), (H,W,C) or (H,W), got {tuple(img.shape)}")
    if c not in (1, 3, 4):
        raise ValueError(f"{what}: {c} channels, expected 1, 3 or 4")
    if h < 1 or w < 1:
        raise ValueError(f"{what}: empty image {tuple(img.shape)}")
    if min(sc, sh, sw) < 0:
        raise ValueError(f"{what}: negative strides are not supported")
    return int(c), int(h), int(w), int(sc), int(sh), int(sw)


class Panel:
    """One image of a grid and its label.

    img: float32 tensor on the GPU, (C,H,W) with layout="chw", (H,W,C) with "hwc", or (H,W); C in {1, 3, 4}; any strides (it
    is read where it is).  label: str or bytes of at most 64 bytes, drawn in `color` (RGB in [0, 1]) as write_text places it;
    thickness >= 2 draws bold.  One "{:.3f}" in the label is filled on the device from value (a float32 tensor on the GPU, its
    first element), formatted as Python formats it."""

    def __init__(self, img, label=None, color=(0.0, 0.0, 0.0), value=None, bottom=False, layout="chw", thickness=2, X=15):
        if isinstance(img, np.ndarray) or not torch.is_tensor(img):
            raise TypeError(f"Panel: expected a tensor on the GPU, got {type(img).__name__}; host arrays have no path in this library "
                            "(move the image to the device and use compose_grid)")
        if img.dtype != torch.float32:
            raise TypeError(f"Panel: the image must be float32, got {img.dtype}")
        self.img, self.layout = img, layout
        self.C, self.h, self.w, self.sc, self.sh, self.sw = _geometry(img, layout, "Panel")
        text = b"" if label is None else (label.encode("utf-8") if isinstance(label, str) else bytes(label))
        if len(text) > MAX_LABEL:
            raise ValueError(f"Panel: a label of {len(text)} bytes, at most {MAX_LABEL} fit ({text[:24]!r}...)")
        n_slots = text.count(SLOT.encode())
        if n_slots > 1:
            raise ValueError(f"Panel: {n_slots} '{SLOT}' slots in {text!r}, a label holds at most one")
        if value is not None:
            if not torch.is_tensor(value):
                raise TypeError(f"Panel: value must be a float32 tensor on the GPU, got {type(value).__name__}")
            if value.dtype != torch.float32:
                raise TypeError(f"Panel: value must be float32, got {value.dtype}")
            if value.numel() < 1:
                raise ValueError("Panel: value is empty")
        if (n_slots == 1) != (value is not None):
            raise ValueError(f"Panel: label {text!r} and value do not fit: a '{SLOT}' slot needs a value cell, and a value cell a slot")
        color = tuple(float(c) for c in color)
        if len(color) != 3:
            raise ValueError(f"Panel: color {color}, expected (r, g, b)")
        self.label, self.color, self.value = text, color, value
        self.flags = (_lib.PANEL_BOTTOM if bottom else 0) | (_lib.PANEL_BOLD if int(thickness) >= 2 else 0)
        self.X = int(X)

    def tensors(self):
        return (self.img, self.value)

    def __repr__(self):
        return f"Panel({self.C}x{self.h}x{self.w}, {self.label!r})"


def _pack(placed, out_h, out_w, mode, channels, order, pad_value, pitch, force_scalar=False):
    """placed: [(Panel, y0, x0)] -> the GridDesc of the launch.  Touches no device."""
    if not 1 <= len(placed) <= MAX_PANELS:
        raise ValueError(f"frame grid: {len(placed)} panels, a launch places 1..{MAX_PANELS}")
    if channels not in (3, 4):
        raise ValueError(f"frame grid: channels={channels}, expected 3 or 4")
    if order not in ("rgb", "bgr"):
        raise ValueError(f"frame grid: order={order!r}, expected 'rgb' or 'bgr'")
    if not (1 <= out_h <= _lib.GRID_MAX_SIDE and 1 <= out_w <= _lib.GRID_MAX_SIDE):
        raise ValueError(f"frame grid: a canvas of {out_h} x {out_w}, each side 1..{_lib.GRID_MAX_SIDE}")
    d = _lib.GridDesc()
    d.n_panels, d.out_H, d.out_W, d.mode, d.channels = len(placed), out_h, out_w, mode, channels
    d.flags = (_lib.GRID_BGR if order == "bgr" else 0) | (_lib.GRID_FORCE_SCALAR if force_scalar else 0)
    d.pad_value, d.pitch = float(pad_value), int(pitch)
    for i, (p, y0, x0) in enumerate(placed):
        if y0 < 0 or x0 < 0 or y0 + p.h > out_h or x0 + p.w > out_w:
            raise ValueError(f"frame grid: panel {i} {p!r} at ({y0}, {x0}) leaves the canvas of {out_h} x {out_w}")
        for j, (q, y1, x1) in enumerate(placed[:i]):
            if y0 < y1 + q.h and y1 < y0 + p.h and x0 < x1 + q.w and x1 < x0 + p.w:
                raise ValueError(f"frame grid: panels {j} {q!r} at ({y1}, {x1}) and {i} {p!r} at ({y0}, {x0}) overlap")
        e = d.panel[i]
        e.src = p.img.data_ptr()
        e.value = p.value.data_ptr() if p.value is not None else None
        e.sc, e.sh, e.sw = p.sc, p.sh, p.sw
        e.C, e.h, e.w, e.y0, e.x0 = p.C, p.h, p.w, int(y0), int(x0)
        e.flags, e.label_len, e.X = p.flags, len(p.label), p.X
        e.color[0], e.color[1], e.color[2] = p.color
        ctypes.memmove(ctypes.addressof(e) + _lib.GridPanel.label.offset, p.label, len(p.label))     # NUL bytes included
    return d


def _layout_rows(rows, pad_even):
    """rows of panels laid out as th.cat(dim=2) inside a row and th.cat(dim=1) across rows -> ([(Panel, y0, x0)], H, W)."""
    if not rows or any(not row for row in rows):
        raise ValueError("compose_grid: expected a non-empty list of non-empty rows of panels")
    placed, y, width = [], 0, None
    for r, row in enumerate(rows):
        x = 0
        for k, p in enumerate(row):
            if not isinstance(p, Panel):
                raise TypeError(f"compose_grid: row {r} entry {k} is {type(p).__name__}, expected a Panel")
            if p.h != row[0].h:
                raise ValueError(f"compose_grid: row {r} entry {k} {p!r} is {p.h} rows high, the row's first panel {row[0]!r} {row[0].h}")
            placed.append((p, y, x))
            x += p.w
        if width is None:
            width = x
        elif x != width:
            raise ValueError(f"compose_grid: row {r} (ending with {row[-1]!r}) is {x} pixels wide, row 0 is {width}")
        y += row[0].h
    if pad_even:
        y, width = y + (y & 1), width + (width & 1)
    return placed, y, width


def _output(out, mode, channels, out_layout, h, w, device):
    """The output tensor (allocated unless given) and its row pitch in bytes (uint8 modes)."""
    u8 = mode in (_lib.GRID_OUT_U8_SAVE_IMAGE, _lib.GRID_OUT_U8_CLIP)
    shape = (channels, h, w) if mode == _lib.GRID_OUT_F32_CHW else (h, w, channels)
    dtype = torch.uint8 if u8 else torch.float32
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=device)
    else:
        if not torch.is_tensor(out) or out.dtype != dtype or tuple(out.shape) != shape:
            raise ValueError(f"frame grid: out must be a {dtype} tensor of shape {shape}, got "
                             f"{(out.dtype, tuple(out.shape)) if torch.is_tensor(out) else type(out).__name__}")
        if u8:
            if out.stride(2) != 1 or out.stride(1) != channels or out.stride(0) < w * channels:
                raise ValueError(f"frame grid: out has strides {out.stride()}: pixels must be dense, rows may be padded")
        elif not out.is_contiguous():
            raise ValueError("frame grid: a float32 out must be contiguous")
    return out, (out.stride(0) if u8 else 0)


def compose_panels(placed, out_size, *, quantize="save_image", order="rgb", channels=3, pad_value=1.0, out=None, out_layout="chw",
                   return_path=False, force_scalar=False):
    """placed: [(Panel, y0, x0)] on a canvas out_size = (H, W): the general form of compose_grid.  Panels must not overlap;
    canvas pixels nobody covers get pad_value."""
    if quantize not in _MODES:
        raise ValueError(f"frame grid: quantize={quantize!r}, expected 'save_image', 'clip' or None")
    if out_layout not in ("chw", "hwc"):
        raise ValueError(f"frame grid: out_layout={out_layout!r}, expected 'chw' or 'hwc'")
    mode = _MODES[quantize]
    if mode is None:
        mode = _lib.GRID_OUT_F32_CHW if out_layout == "chw" else _lib.GRID_OUT_F32_HWC
    placed = list(placed)
    h, w = int(out_size[0]), int(out_size[1])
    d = _pack(placed, h, w, mode, channels, order, pad_value, 0, force_scalar)
    tensors = [t for p, _, _ in placed for t in p.tensors()]
    _lib.require_cuda(*tensors, out)
    out, pitch = _output(out, mode, channels, out_layout, h, w, placed[0][0].img.device)
    d.pitch = pitch
    path = ctypes.c_int32(0)
    check(_lib.lib().d3ga_frame_grid(ctypes.byref(d), out.data_ptr(), ctypes.byref(path), stream_handle()), "d3ga_frame_grid")
    return (out, "vector" if path.value else "scalar") if return_path else out


def compose_grid(rows, *, quantize="save_image", order="rgb", channels=3, pad_even=True, pad_value=1.0, out=None, out_layout="chw",
                 return_path=False, force_scalar=False):
    """rows: a list of lists of Panel, laid out as th.cat(dim=2) inside a row and th.cat(dim=1) across rows; heights inside a row
    and the widths of the rows must agree (ValueError names the panel).  pad_even: one row / column of pad_value where the
    height / width is odd (test.py:176-179).

    quantize "save_image" | "clip": uint8 (H, W, channels) in `order` -- torchvision's mul(255).add_(0.5).clamp_(0, 255) |
    train.py:365's np.clip(x * 255, 0, 255), a NaN gives 0.  None: float32, (channels, H, W) or with out_layout="hwc"
    (H, W, channels), unquantised.  channels 3 | 4: a source without alpha has alpha 1; text leaves alpha alone.

    One launch, no synchronisation; with out= no allocation either, so the call can sit in a captured graph (the label bytes
    and panel addresses are then the graph's; a value cell is read on every replay).  return_path: also "vector" | "scalar",
    the kernel the launch took (both give the same bytes)."""
    placed, h, w = _layout_rows(rows, pad_even)
    return compose_panels(placed, (h, w), quantize=quantize, order=order, channels=channels, pad_value=pad_value, out=out,
                          out_layout=out_layout, return_path=return_path, force_scalar=force_scalar)


def to_uint8(img, *, layout="chw", quantize="save_image", order="rgb", channels=None, pad_even=False, out=None):
    """A single image -> uint8 (H, W, channels): save_image's conversion of test.py:182-195 (prediction, heatmap, the RGBA
    ground_truth).  channels defaults to 4 for a four-channel image, else 3."""
    p = Panel(img, layout=layout)
    return compose_grid([[p]], quantize=quantize, order=order, channels=channels or (4 if p.C == 4 else 3), pad_even=pad_even, out=out)


def write_text(img, text, fontColor=(0, 0, 0), thickness=2, bottom=False, X=15, layout="chw"):
    """utils/text_helpers.py:27-50 for a device tensor: a NEW float32 image in the layout of `img` with `text` drawn on it; the
    input is not touched, and pixels the text does not reach keep their bits.  A one-channel image comes back with three."""
    if not torch.is_tensor(img):
        raise TypeError(f"write_text: expected a tensor on the GPU, got {type(img).__name__}; this library has no CPU path -- "
                        "move the image to the device, or draw and assemble the whole frame with compose_grid")
    p = Panel(img, label=text, color=fontColor, bottom=bottom, layout=layout, thickness=thickness, X=X)
    return compose_grid([[p]], quantize=None, channels=4 if p.C == 4 else 3, pad_even=False, out_layout=layout)


class _Handle:
    """One submitted image: numpy() waits for ITS copy only.  Safe to use from any thread."""

    def __init__(self, writer, slot, shape):
        self._writer, self._slot, self._shape, self._data = writer, slot, shape, None

    def _detach_locked(self):
        """With the slot's lock held: wait for the copy, take the image out of the pinned buffer, free the slot."""
        if self._data is None:
            w, n = self._writer, int(np.prod(self._shape))
            w._events[self._slot].synchronize()
            self._data = w._buffers[self._slot][:n].numpy().reshape(self._shape).copy()
            if w._owners[self._slot] is self:
                w._owners[self._slot] = None
        return self._data

    def done(self):
        """True once numpy() would not wait for the device."""
        if self._data is not None:
            return True
        with self._writer._locks[self._slot]:
            return self._data is not None or self._writer._events[self._slot].query()

    def numpy(self):
        """The (H, W, C) uint8 array, the handle's own: a host copy out of the pinned slot, which is free afterwards."""
        if self._data is not None:
            return self._data
        with self._writer._locks[self._slot]:
            return self._detach_locked()


class _PngHandle:
    """One submitted PNG buffer: tobytes() / save() wait for ITS copy only.  Safe to use from any thread."""

    def __init__(self, writer, slot, nbytes):
        self._writer, self._slot, self._nbytes, self._data = writer, slot, nbytes, None

    def _detach_locked(self):
        """With the slot's lock held: wait for the copy, read the length word, take the file's bytes out, free the slot."""
        if self._data is None:
            w = self._writer
            w._events[self._slot].synchronize()
            host = w._buffers[self._slot][:self._nbytes].numpy()
            n = int(host[:8].view(np.uint64)[0])
            if n > self._nbytes - 8:
                raise _lib.D3GAError(f"submit_png: the length word says {n} bytes, the buffer holds {self._nbytes - 8}: nothing was "
                                     "encoded into it")
            self._data = host[8:8 + n].tobytes()
            if w._owners[self._slot] is self:
                w._owners[self._slot] = None
        return self._data

    def done(self):
        """True once tobytes() would not wait for the device."""
        if self._data is not None:
            return True
        with self._writer._locks[self._slot]:
            return self._data is not None or self._writer._events[self._slot].query()

    def tobytes(self):
        """The PNG file's bytes, the handle's own; the pinned slot is free afterwards."""
        if self._data is not None:
            return self._data
        with self._writer._locks[self._slot]:
            return self._detach_locked()

    def save(self, path):
        """Write the file: what the save pool's thread calls."""
        data = self.tobytes()
        with open(path, "wb") as f:
            f.write(data)


class GridWriter:
    """A ring of `depth` pinned host buffers between the frame loop and the threads that encode images.

    submit(t) enqueues ONE asynchronous device -> host copy of a uint8 tensor on the current stream, records an event and
    returns a handle at once; handle.numpy() -- called by whoever saves the image, in any thread -- waits for that event only
    and returns the (H, W, C) uint8 array.  That array is a second, host-to-host copy out of the pinned slot (the price of
    freeing the slot at once; it runs in the caller of numpy(), i.e. in the save pool).  When all `depth` slots hold images nobody
    has taken yet, submit waits for the OLDEST one and takes it out for its handle -- then that host copy runs in the frame loop
    -- before the slot is reused: nothing is ever overwritten.  Choose `depth` so that the ring is rarely full.

    Threads: every slot has a lock that covers the wait, the copy out and the hand-over of the slot in numpy(), and the reuse
    of the slot in submit(); a handle frees a slot only while it still owns it."""

    def __init__(self, depth=4):
        if int(depth) < 1:
            raise ValueError(f"GridWriter: depth={depth}, expected at least 1")
        self.depth = int(depth)
        self._buffers, self._events, self._owners = [None] * self.depth, [None] * self.depth, [None] * self.depth
        self._locks = [threading.Lock() for _ in range(self.depth)]
        self._ring = threading.Lock()
        self._next = 0

    def submit(self, image):
        if not torch.is_tensor(image) or image.dtype != torch.uint8:
            raise TypeError(f"GridWriter.submit: expected a uint8 tensor on the GPU, got "
                            f"{image.dtype if torch.is_tensor(image) else type(image).__name__}")
        _lib.require_cuda(image)
        with self._ring:
            slot, self._next = self._next, (self._next + 1) % self.depth
        with self._locks[slot]:
            if self._owners[slot] is not None:
                self._owners[slot]._detach_locked()
            n = image.numel()
            if self._buffers[slot] is None or self._buffers[slot].numel() < n:
                self._buffers[slot] = torch.empty(n, dtype=torch.uint8, pin_memory=True)
            if self._events[slot] is None:
                self._events[slot] = torch.cuda.Event()
            self._buffers[slot][:n].view(image.shape).copy_(image, non_blocking=True)
            self._events[slot].record()
            handle = _Handle(self, slot, tuple(image.shape))
            self._owners[slot] = handle
        return handle

    def submit_png(self, buf):
        """A PngBuffer (d3ga_amd.png.encode_png) instead of an image: ONE asynchronous copy of [length word | PNG bytes up to the
        capacity] into a pinned slot of the same ring -- the length is not known on the host, and reading it first would be a
        synchronisation.  The handle's tobytes() / save(path) wait for that copy only and take bytes[:length]."""
        from .png import PngBuffer
        if not isinstance(buf, PngBuffer):
            raise TypeError(f"GridWriter.submit_png: expected a PngBuffer, got {type(buf).__name__}")
        _lib.require_cuda(buf.buffer)
        with self._ring:
            slot, self._next = self._next, (self._next + 1) % self.depth
        with self._locks[slot]:
            if self._owners[slot] is not None:
                self._owners[slot]._detach_locked()
            n = buf.buffer.numel()
            if self._buffers[slot] is None or self._buffers[slot].numel() < n:
                self._buffers[slot] = torch.empty(n, dtype=torch.uint8, pin_memory=True)
            if self._events[slot] is None:
                self._events[slot] = torch.cuda.Event()
            self._buffers[slot][:n].copy_(buf.buffer, non_blocking=True)
            self._events[slot].record()
            handle = _PngHandle(self, slot, n)
            self._owners[slot] = handle
        return handle
