"""The PNG encoder (d3ga_amd/png.py): an independent decoder out of the standard library and numpy, the g++
build of csrc/png_math.h (tests/hostcheck/pngcheck.cpp) -- the text the kernels run -- behind ctypes, and the cases both the
host and the GPU tests run."""
import ctypes
import os
import struct
import subprocess
import zlib

import numpy as np

from conftest import ROOT

ADAPTIVE = 5
FILTERS = {"adaptive": ADAPTIVE, 0: 0, 1: 1, 2: 2, 3: 3, 4: 4}
SIGNATURE = b"\x89PNG\r\n\x1a\n"
TYPE_FIXED, TYPE_DYNAMIC = 1, 2
HEAD_BYTES, TAIL_BYTES = 47, 30


# ---- the g++ build ------------------------------------------------------------------------------------------------------------
class StripInfo(ctypes.Structure):
    """struct PngStripInfo (csrc/png_math.h)"""
    _fields_ = [(n, ctypes.c_int32) for n in ("type", "depth", "hlit", "hclen", "nused")] + \
               [(n, ctypes.c_uint64) for n in ("dyn_bits", "fix_bits", "hdr_bits", "seg_bytes")] + \
               [("llen", ctypes.c_uint8 * 288), ("cllen", ctypes.c_uint8 * 19)]


def pngcheck():
    src = os.path.join(ROOT, "tests", "hostcheck", "pngcheck.cpp")
    out_dir = os.path.join(ROOT, "tests", "hostcheck", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libpngcheck.so")
    deps = [src, os.path.join(ROOT, "include", "d3ga.h"), os.path.join(ROOT, "d3ga_amd", "csrc", "png_math.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", so])
    lib = ctypes.CDLL(so)
    i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    lib.hc_png_plan.argtypes = [i32] * 4 + [vp]
    lib.hc_png_check.argtypes = [i32, i32, i32, i64, i32, i32, vp, vp, i64, vp, i64]
    lib.hc_png_encode.argtypes = [i32, i32, i32, i64, i32, i32, vp, vp, i64, vp, i64, vp, vp]
    lib.hc_png_lengths.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp]
    lib.hc_png_header.argtypes = [vp] * 5
    lib.hc_png_crc.restype = ctypes.c_uint32
    lib.hc_png_crc.argtypes = [vp, i64]
    lib.hc_png_crc_shift.restype = ctypes.c_uint32
    lib.hc_png_crc_shift.argtypes = [ctypes.c_uint32, ctypes.c_uint64]
    lib.hc_png_default_rows.argtypes = [i32] * 3
    return lib


_LIB = []


def lib():
    if not _LIB:
        _LIB.append(pngcheck())
    return _LIB[0]


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_plan(H, W, C, rows=0):
    """dict of the plan's sizes, or the status"""
    o = np.zeros(7, np.int64)
    st = lib().hc_png_plan(H, W, C, rows, _p(o))
    if st != 0:
        return st
    return dict(zip(("rows", "strips", "n_full", "slot", "capacity", "scratch_bytes", "use_lds"), (int(v) for v in o)))


def image_pitch(img):
    """(H, W, C, pitch) of a uint8 array whose pixels are dense and whose rows may be padded"""
    H, W, C = img.shape
    assert img.dtype == np.uint8 and img.strides[2] == 1 and img.strides[1] == C and img.strides[0] >= W * C, img.strides
    return H, W, C, img.strides[0]


class HostPng:
    """What the g++ build makes of an image: .data (the file's bytes), .capacity, .info (a StripInfo per strip), .filtered"""


def host_encode(img, filter="adaptive", rows=0):
    H, W, C, pitch = image_pitch(img)
    plan = host_plan(H, W, C, rows)
    assert isinstance(plan, dict), plan
    out = np.full(8 + plan["capacity"], 0xAB, np.uint8)
    scratch = np.zeros(plan["scratch_bytes"] + 16, np.uint8)
    scratch = scratch[(-scratch.ctypes.data) % 16:][:plan["scratch_bytes"]]
    info = (StripInfo * plan["strips"])()
    filtered = np.zeros(H * (W * C + 1), np.uint8)
    st = lib().hc_png_encode(H, W, C, pitch, FILTERS[filter], rows, ctypes.c_void_p(img.ctypes.data), _p(out), plan["capacity"],
                             _p(scratch), plan["scratch_bytes"], ctypes.cast(info, ctypes.c_void_p), _p(filtered))
    assert st == 0, st
    n = int(out[:8].view(np.uint64)[0])
    assert n <= plan["capacity"]
    assert (out[8 + n:] == 0xAB).all(), "the host build wrote beyond the length"
    r = HostPng()
    r.data, r.capacity, r.info, r.filtered, r.plan = out[8:8 + n].tobytes(), plan["capacity"], list(info), filtered, plan
    return r


def host_lengths(freq, maxbits):
    """(lengths, depth of the unlimited code) by the header's code construction"""
    freq = np.ascontiguousarray(freq, np.uint32)
    out = np.zeros(len(freq), np.uint8)
    depth = lib().hc_png_lengths(_p(freq), len(freq), maxbits, _p(out))
    return out, depth


def host_header(freq286):
    """the block header of a histogram: (literal/length lengths, code-length lengths, code-length counts, unlimited depth of the
    code-length code, header bits)"""
    freq = np.ascontiguousarray(freq286, np.uint32)
    llen, cllen, clfreq, depth = np.zeros(286, np.uint8), np.zeros(19, np.uint8), np.zeros(19, np.uint32), ctypes.c_int32(0)
    bits = lib().hc_png_header(_p(freq), _p(llen), _p(cllen), _p(clfreq), ctypes.byref(depth))
    return llen, cllen, clfreq, depth.value, bits


def kraft(lengths):
    """sum of 2^-l over the used codes, as an exact fraction of 2^-32"""
    return sum(1 << (32 - int(l)) for l in lengths if l)


# ---- the decoder --------------------------------------------------------------------------------------------------------------
def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def unfilter(filtered, H, W, C):
    """PNG specification 9.2: filtered bytes (H, 1 + W C) -> (H, W, C) and the filter types"""
    rows = np.frombuffer(filtered, np.uint8).reshape(H, 1 + W * C)
    out = np.zeros((H, W, C), np.int64)
    types = rows[:, 0].copy()
    for y in range(H):
        line = rows[y, 1:].reshape(W, C).astype(np.int64)
        up = out[y - 1] if y else np.zeros((W, C), np.int64)
        t = types[y]
        assert t <= 4, f"row {y}: filter type {t}"
        if t == 0:
            out[y] = line
        elif t == 2:
            out[y] = (line + up) & 255
        else:
            left, upleft = np.zeros(C, np.int64), np.zeros(C, np.int64)
            for x in range(W):
                pred = left if t == 1 else (left + up[x]) >> 1 if t == 3 else paeth(left, up[x], upleft)
                left = (line[x] + pred) & 255
                out[y, x] = left
                upleft = up[x]
    return out.astype(np.uint8), types


class Decoded:
    """.image (H, W, C), .filters (H,), .filtered (bytes), .segments [bytes of each strip's IDAT], .strip_bytes [filtered bytes each
    inflates to alone], .types [block type of each segment: 1 fixed, 2 dynamic]"""


def decode(data):
    assert data[:8] == SIGNATURE
    chunks, at = [], 8
    while at < len(data):
        n, = struct.unpack(">I", data[at:at + 4])
        name, body = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        crc, = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        assert zlib.crc32(name + body) == crc, f"chunk {len(chunks)} {name}: CRC"
        chunks.append((name, body))
        at += 12 + n
    assert at == len(data), "bytes behind the last chunk"
    names = [c[0] for c in chunks]
    assert names[0] == b"IHDR" and names[-1] == b"IEND" and len(chunks[-1][1]) == 0, names
    assert len(chunks) >= 5 and all(n == b"IDAT" for n in names[1:-1]), names
    W, H, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0) and ctype in (0, 2, 6)
    C = {0: 1, 2: 3, 6: 4}[ctype]
    assert chunks[1][1] == b"\x78\x01", chunks[1][1]
    last = chunks[-2][1]
    assert len(last) == 6 and last[:2] == b"\x03\x00", last
    d = Decoded()
    d.segments = [c[1] for c in chunks[2:-2]]
    d.filtered = zlib.decompress(b"".join(c[1] for c in chunks[1:-1]))       # verifies the Adler-32 and the codes
    assert len(d.filtered) == H * (1 + W * C)
    d.adler, = struct.unpack(">I", last[2:])
    assert d.adler == zlib.adler32(d.filtered)
    d.strip_bytes, d.types, alone = [], [], []
    for seg in d.segments:
        assert seg[-4:] == b"\x00\x00\xff\xff", "a segment ends with the empty stored block of a sync flush"
        assert seg[0] & 1 == 0, "BFINAL inside a strip"
        d.types.append((seg[0] >> 1) & 3)
        o = zlib.decompressobj(-15)
        part = o.decompress(seg)
        assert not o.unused_data and not o.eof
        alone.append(part)
        d.strip_bytes.append(len(part))
    assert b"".join(alone) == d.filtered, "every segment inflates alone: no match crosses a strip"
    d.image, d.filters = unfilter(d.filtered, H, W, C)
    return d


def filter_rows(img):
    """(5, H, W C) uint8: every row under every filter type, by the PNG specification"""
    H, W, C = img.shape
    x = img.astype(np.int64)
    a = np.zeros_like(x)
    a[:, 1:] = x[:, :-1]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, 1:] = x[:-1, :-1]
    preds = [np.zeros_like(x), a, b, (a + b) >> 1, paeth(a, b, c)]
    return np.stack([((x - p) & 255).astype(np.uint8).reshape(H, W * C) for p in preds])


def adaptive_choice(img):
    """the rule, brute force: per row the type with the smallest sum of |int8|, ties to the lower type"""
    f = filter_rows(np.ascontiguousarray(img)).astype(np.int64)
    cost = np.where(f < 128, f, 256 - f).sum(axis=2)          # (5, H)
    return np.argmin(cost, axis=0).astype(np.uint8)           # argmin takes the first minimum


def zlib_rle_size(filtered, strip_bytes):
    """the yardstick: zlib level 6, Z_RLE, every strip on its own, ended by a sync flush"""
    total, at = 0, 0
    for n in strip_bytes:
        o = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_RLE)
        total += len(o.compress(filtered[at:at + n]) + o.flush(zlib.Z_SYNC_FLUSH))
        at += n
    return total


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.default_rng(seed)


def noise(H, W, C, seed=0):
    return _rng(seed).integers(0, 256, (H, W, C), dtype=np.uint8)


def ramp(H, W, C):
    y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(C), indexing="ij")
    return ((3 * x + 5 * y + 40 * c) & 255).astype(np.uint8)


def padded(img, extra=13):
    """the same pixels with rows `extra` bytes further apart, the gap filled with 0x5A"""
    H, W, C = img.shape
    base = np.full((H, W * C + extra), 0x5A, np.uint8)
    base[:, :W * C] = img.reshape(H, W * C)
    return np.lib.stride_tricks.as_strided(base, (H, W, C), (base.strides[0], C, 1))


def runs_row():
    """one row: runs of every length 1..300, the byte changing from run to run"""
    out, v = [], 1
    for n in range(1, 301):
        out.append(np.full(n, v, np.uint8))
        v = v % 250 + 1
    return np.concatenate(out).reshape(1, -1, 1)


def fibonacci_counts():
    f = [1, 1]
    while f[-1] < 1597:
        f.append(f[-1] + f[-2])
    return f                                 # 17 counts, 4180 in all


def fibonacci_row():
    """one row of 4179 bytes: with the filter byte 0 the literal counts are 1, 1, 2, 3, ... 1597, and no byte equals its neighbour"""
    counts = fibonacci_counts()[1:]         # the first 1 is the filter byte
    syms = np.concatenate([np.full(c, i + 1, np.uint8) for i, c in sorted(enumerate(counts), key=lambda t: -t[1])])
    row = np.zeros(len(syms), np.uint8)
    half = (len(syms) + 1) // 2
    row[0::2] = syms[:half]
    row[1::2] = syms[half:]
    assert (row[1:] != row[:-1]).all() and row[0] != 0
    return row.reshape(1, -1, 1)


def paeth_ties():
    """a = b = c on a flat region, and pa = pb where the left and upper neighbours differ from the corner by the same amount"""
    img = np.full((6, 8, 1), 90, np.uint8)
    img[2, :, 0] = [10, 30, 10, 30, 50, 70, 50, 30]
    img[3, :, 0] = [30, 50, 30, 10, 70, 90, 70, 50]
    img[4, :, 0] = [30, 10, 30, 50, 90, 70, 90, 70]
    return img


def cases():
    """[(name, image, filter, rows_per_strip)]: small enough that each runs in well under a second"""
    out = [("1x1x1", np.array([[[7]]], np.uint8), "adaptive", 0),
           ("7x5x3", noise(7, 5, 3, 1), "adaptive", 0),
           ("single_strip", ramp(33, 17, 4), "adaptive", 33),
           ("pitch", padded(ramp(9, 11, 3)), "adaptive", 2),
           ("pitch_noise", padded(noise(9, 11, 4, 2), 5), 4, 0)]
    for rows in (1, 2, 3, 0):
        out.append((f"33x17x4_r{rows}", (ramp(33, 17, 4) + (noise(33, 17, 4, 3) >> 6)).astype(np.uint8), "adaptive", rows))
    for f in (0, 1, 2, 3, 4, "adaptive"):
        out.append((f"noise_f{f}", noise(9, 11, 3, 4), f, 4))
        out.append((f"ramp_f{f}", ramp(9, 11, 3), f, 4))
    out += [("paeth_ties", paeth_ties(), 4, 0),
            ("average_carry", np.full((5, 9, 3), 200, np.uint8), 3, 2),
            ("runs", runs_row(), 0, 0),
            ("runs_two_rows_one_strip", np.concatenate([runs_row(), runs_row()]), 0, 2),       # 90302 bytes: past the LDS stage
            ("zeros", np.zeros((16, 64, 1), np.uint8), 0, 4),
            ("zeros_sub", np.zeros((16, 64, 1), np.uint8), 1, 4),
            ("zeros_row_strips", np.zeros((5, 700, 1), np.uint8), 0, 1),
            ("all_literals", np.arange(1, 256, dtype=np.uint8).reshape(1, 255, 1), 0, 0),
            ("noise_4k", noise(1, 4095, 1, 5), 0, 0),
            ("one_value", np.full((8, 64, 1), 7, np.uint8), 0, 0),
            ("fibonacci", fibonacci_row(), 0, 0),
            ("adler_ff", np.full((40, 600, 1), 255, np.uint8), 0, 8),
            ("adler_ff_6010", np.full((40, 600, 1), 255, np.uint8), 0, 10)]
    return out


CASES = cases()
CASE_IDS = [c[0] for c in CASES]
_HOST = {}


def host_case(name):
    """the g++ build's file for a case, computed once and shared"""
    if name not in _HOST:
        _, img, f, rows = CASES[CASE_IDS.index(name)]
        _HOST[name] = host_encode(img, f, rows)
    return _HOST[name]


def body_on_white(H=256, W=256, seed=7):
    """the issue's synthetic frame: a white background with a textured body"""
    y, x = np.mgrid[0:H, 0:W]
    body = ((x - W / 2) / (0.28 * W)) ** 2 + ((y - H / 2) / (0.42 * H)) ** 2 < 1
    r = _rng(seed)
    tex = (128 + 60 * np.sin(x / 7.0)[..., None] * np.cos(y / 5.0)[..., None] + r.normal(0, 12, (H, W, 3))).clip(0, 255)
    return np.where(body[..., None], tex, 255).astype(np.uint8)
