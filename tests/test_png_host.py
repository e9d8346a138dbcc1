"""The PNG encoder on the CPU: the g++ build of csrc/png_math.h -- the text the kernels run, one "thread" after
the other -- against an independent decoder (tests/png_ref.py), numpy restatements of the filter and token rules, and zlib.
tests/test_gpu_png.py holds the kernels to the same bytes."""
import ctypes
import io
import zlib

import numpy as np
import pytest
import torch

import png_ref as R


def strip_sizes(H, W, C, rows):
    n = rows * (W * C + 1)
    return [min(n, (H - s * rows) * (W * C + 1)) for s in range((H + rows - 1) // rows)]


def rle_tokens(f):
    """the token rule restated: a maximal run is its first byte, then matches of 258 cut greedily from the second byte on; a
    remainder of 3 or more is a match, of 1 or 2 is literals -> [('lit', v) | ('run', length)]"""
    out, i, n = [], 0, len(f)
    while i < n:
        e = i + 1
        while e < n and f[e] == f[i]:
            e += 1
        out.append(("lit", f[i]))
        rest = e - i - 1
        while rest >= 3:
            out.append(("run", min(rest, 258)))
            rest -= min(rest, 258)
        out += [("lit", f[i])] * rest
        i = e
    return out


LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]       # RFC 1951, 3.2.5


def fixed_bits(tokens):
    """bits of a fixed-table block of these tokens: header, tokens with distance 1 (5 bits), end of block (RFC 1951, 3.2.6)"""
    bits = 3 + 7
    for kind, v in tokens:
        if kind == "lit":
            bits += 8 if v < 144 else 9
        else:
            k = max(i for i, b in enumerate(LENGTH_BASE) if b <= v)
            bits += (7 if 257 + k < 280 else 8) + LENGTH_EXTRA[k] + 5
    return bits


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_host_file_decodes_to_the_image(name):
    _, img, f, rows = R.CASES[R.CASE_IDS.index(name)]
    h = R.host_case(name)
    d = R.decode(h.data)
    H, W, C = img.shape
    assert d.image.shape == img.shape and (d.image == img).all()
    assert len(h.data) <= h.capacity
    assert d.strip_bytes == strip_sizes(H, W, C, h.plan["rows"]), "a segment per strip, each inflating to its own rows"
    assert d.filtered == h.filtered.tobytes()
    # the capacity formula of the header, restated
    assert h.capacity == 77 + sum((9 * n + 7) // 8 + 8 + 12 for n in d.strip_bytes)
    # filters: the forced type, or the brute-force restatement of the adaptive rule, row by row
    want = R.adaptive_choice(img) if f == "adaptive" else np.full(H, f, np.uint8)
    assert (d.filters == want).all(), (d.filters, want)
    rows_f = R.filter_rows(np.ascontiguousarray(img))
    got = np.frombuffer(d.filtered, np.uint8).reshape(H, 1 + W * C)[:, 1:]
    assert (got == rows_f[want, np.arange(H)]).all()
    # tokens and the choice of block: the smaller of the two exact counts, ties to the fixed block, as the segment's bits say
    at = 0
    for s, (info, seg) in enumerate(zip(h.info, d.segments)):
        part = d.filtered[at:at + d.strip_bytes[s]]
        at += d.strip_bytes[s]
        assert info.fix_bits == fixed_bits(rle_tokens(part)), f"strip {s}: the tokens are not the rule's"
        want_type = R.TYPE_DYNAMIC if info.dyn_bits < info.fix_bits else R.TYPE_FIXED
        assert info.type == want_type == d.types[s]
        assert len(seg) == info.seg_bytes == (min(info.dyn_bits, info.fix_bits) + 3 + 7) // 8 + 4
        assert len(seg) <= (info.fix_bits + 3 + 7) // 8 + 4, "no segment is larger than its fixed-table encoding"
        assert len(seg) <= (9 * len(part) + 7) // 8 + 8


@pytest.mark.parametrize("name", ["33x17x4_r2", "7x5x3", "1x1x1", "adler_ff", "pitch"])
def test_pil_opens_the_file(name):
    Image = pytest.importorskip("PIL.Image")
    _, img, _, _ = R.CASES[R.CASE_IDS.index(name)]
    got = np.array(Image.open(io.BytesIO(R.host_case(name).data)))
    assert (got.reshape(img.shape) == img).all()


def test_runs_of_every_length_cut_as_the_rule_says():
    f = R.host_case("runs").filtered.tobytes()
    toks = rle_tokens(f)
    runs = [v for k, v in toks if k == "run"]
    assert 3 in runs and 258 in runs and max(runs) == 258
    # run lengths 259, 260 and 261 in the image: a literal and one match of 258, then nothing | one | two literals; 262: a match of 3
    assert rle_tokens(b"\x05" * 259) == [("lit", 5), ("run", 258)]
    assert rle_tokens(b"\x05" * 261) == [("lit", 5), ("run", 258), ("lit", 5), ("lit", 5)]
    assert rle_tokens(b"\x05" * 262) == [("lit", 5), ("run", 258), ("run", 3)]
    assert rle_tokens(b"\x05" * 3) == [("lit", 5)] * 3
    # the zero image: the filter byte is 0 too, so a strip is ONE run; with Sub the filter byte 1 breaks it at every row
    z, zs = R.host_case("zeros"), R.host_case("zeros_sub")
    assert rle_tokens(z.filtered.tobytes()[:4 * 65]) == [("lit", 0), ("run", 258), ("lit", 0)]      # 260 zeros, rows and all
    assert [k for k, _ in rle_tokens(zs.filtered.tobytes()[:4 * 65])].count("lit") == 8
    assert len(z.data) < len(zs.data)
    # a run that spans a strip boundary is cut there: every strip of zeros_row_strips starts with its own literal
    d = R.decode(R.host_case("zeros_row_strips").data)
    assert d.strip_bytes == [701] * 5 and len(set(d.segments)) == 1


def test_table_cases():
    lit = R.host_case("all_literals")
    assert R.decode(lit.data).types == [R.TYPE_FIXED] and lit.info[0].nused == 257
    nz = R.host_case("noise_4k")
    assert nz.info[0].type == (R.TYPE_DYNAMIC if nz.info[0].dyn_bits < nz.info[0].fix_bits else R.TYPE_FIXED)
    one = R.host_case("one_value")
    assert one.info[0].type == R.TYPE_DYNAMIC and one.info[0].nused >= 3


def test_length_limit_of_the_literal_code():
    h = R.host_case("fibonacci")
    info = h.info[0]
    assert len(h.filtered) == 4180
    counts = np.bincount(h.filtered, minlength=256)
    assert sorted(int(c) for c in counts if c) == sorted(R.fibonacci_counts())
    assert info.depth > 15, "the unlimited Huffman code of this histogram is deeper than 15: the limiter ran"
    assert info.type == R.TYPE_DYNAMIC
    llen = np.array(info.llen[:286])
    assert llen.max() == 15 and R.kraft(llen) == 1 << 32
    assert ((llen > 0) == (np.append(counts, [1] + [0] * 29) > 0)).all()
    # the header function alone, same histogram
    freq = np.append(counts, [1] + [0] * 29)
    lim, depth = R.host_lengths(freq, 15)
    assert depth == info.depth and (lim == llen).all()
    # without a limit in reach the lengths are Huffman's: the weighted length is the minimum zlib would reach too
    small = np.array([5, 9, 12, 13, 16, 45], np.uint32)
    lens, depth = R.host_lengths(small, 15)
    assert depth == 4 and sorted(lens) == [1, 3, 3, 3, 4, 4] and int((small * lens).sum()) == 224


def deep_header_histogram():
    """a literal/length histogram whose code lengths occur 1, 1, 2, 3, 5, 8, 13, 21, 34, 55 times, no four equal in a row"""
    counts = {10: 1, 2: 1, 8: 2, 12: 3, 5: 5, 13: 8, 14: 13, 6: 21, 3: 34, 11: 55}
    groups = [[l] * c for l, c in sorted(counts.items(), key=lambda t: -t[1])]
    seq = []
    while any(groups):
        for g in groups:
            if g:
                seq.append(g.pop())
    f = np.zeros(286, np.uint32)
    for s, l in enumerate(seq):
        f[s] = 1 << (16 - l)
    f[256] = 1
    return f


def test_length_limit_of_the_code_length_code():
    lens, depth = R.host_lengths(R.fibonacci_counts() + [2584, 4181], 7)
    assert depth > 7 and lens.max() == 7 and lens.min() >= 1 and R.kraft(lens) == 1 << 32
    llen, cllen, clfreq, cl_depth, bits = R.host_header(deep_header_histogram())
    assert cl_depth > 7, "the unlimited code-length code of this header is deeper than 7: the limiter ran"
    assert cllen.max() == 7 and R.kraft(cllen) == 1 << 32 and ((cllen > 0) == (clfreq > 0)).all()
    assert R.kraft(llen) == 1 << 32 and llen.max() <= 15
    hclen = max(k for k, s in enumerate([16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]) if cllen[s]) + 1
    extra = {16: 2, 17: 3, 18: 7}
    assert bits == 17 + 3 * max(hclen, 4) + sum(int(clfreq[s]) * (int(cllen[s]) + extra.get(s, 0)) for s in range(19))


def test_checksums():
    for name in ("adler_ff", "adler_ff_6010"):
        h = R.host_case(name)
        d = R.decode(h.data)                  # asserts Adler-32 == zlib.adler32(filtered) and every chunk's CRC
        assert d.adler == zlib.adler32(h.filtered.tobytes()) and (h.filtered.reshape(40, 601)[:, 1:] == 255).all()
    assert max(R.decode(R.host_case("adler_ff_6010").data).strip_bytes) > 5552
    rng = np.random.default_rng(0)
    for na, nb in ((0, 5), (5, 0), (1, 1), (100, 3000), (4097, 65536)):
        a, b = rng.integers(0, 256, na, dtype=np.uint8), rng.integers(0, 256, nb, dtype=np.uint8)
        ca = R.lib().hc_png_crc(R._p(a), na) if na else 0
        assert ca == zlib.crc32(a.tobytes())
        assert R.lib().hc_png_crc_shift(ca, nb) ^ zlib.crc32(b.tobytes()) == zlib.crc32(a.tobytes() + b.tobytes())


# encoder / zlib (level 6, Z_RLE, per strip, sync flush) on the same filtered bytes.  The bytes are deterministic; the bar is the
# measured excess rounded up to the next whole percent (measured 0.9999, 1.0006 and 1.0056 -- zlib stores noise
# uncompressed, and this stream has no stored block; a table per strip loses next to nothing against zlib's block splitting)
SIZE_CASES = {"body_on_white": (lambda: R.body_on_white(256, 256), 8, 1.00),
              "ramp": (lambda: R.ramp(256, 256, 3), 8, 1.01),
              "noise": (lambda: R.noise(256, 256, 3, 11), 8, 1.01)}


@pytest.mark.parametrize("name", list(SIZE_CASES))
def test_size_against_zlib_rle(name):
    make, rows, bar = SIZE_CASES[name]
    img = make()
    h = R.host_encode(img, "adaptive", rows)
    sizes = strip_sizes(256, 256, 3, rows)
    ours = sum(i.seg_bytes for i in h.info)
    ref = R.zlib_rle_size(h.filtered.tobytes(), sizes)
    print(f"{name}: encoder {ours} zlib {ref} ratio {ours / ref:.4f} file {len(h.data)}")
    assert ours <= bar * ref, (ours, ref, ours / ref)
    assert len(h.data) <= h.capacity
    assert (R.decode(h.data).image == img).all()


def test_plan_and_default_rows():
    assert R.lib().hc_png_default_rows(1080, 1920, 3) == 32768 // 5761 == 5
    assert R.lib().hc_png_default_rows(3, 1920, 3) == 3 and R.lib().hc_png_default_rows(100, 100000, 4) == 1
    p = R.host_plan(1080, 1920, 3)
    assert p["rows"] == 5 and p["strips"] == 216 and p["use_lds"] == 1
    assert R.host_plan(2, 45150, 1, 2)["use_lds"] == 0
    import d3ga_amd
    L = d3ga_amd.lib()
    for H, W, C, rows in ((1080, 1920, 3, 0), (747, 1022, 4, 0), (33, 17, 4, 3), (1, 1, 1, 0), (2, 45150, 1, 2)):
        p, scratch = R.host_plan(H, W, C, rows), ctypes.c_int64(0)
        assert L.d3ga_png_capacity(H, W, C, rows, ctypes.byref(scratch)) == p["capacity"] and scratch.value == p["scratch_bytes"]


def test_entry_points_refuse_bad_arguments_no_gpu_needed():
    """the status table of d3ga_png_check / d3ga_png_encode (include/d3ga.h), decided before any HIP call: every pointer is a
    made-up address that is never read; the Python layer raises on the same before it touches a device."""
    import d3ga_amd
    from d3ga_amd import PngBuffer, encode_png
    L = d3ga_amd.lib()
    OK, E_NULL, E_SIZE, E_CONFIG, E_CAPACITY = 0, -1, -2, -3, -4
    img, out, scr, big = 0x10000, 0x20008, 0x30000, 1 << 40
    good = dict(H=9, W=11, C=3, pitch=33, filter=5, rows=0, img=img, out=out, out_bytes=big, scratch=scr, scratch_bytes=big)

    def status(entry, **kw):
        a = dict(good, **kw)
        args = [a[k] for k in ("H", "W", "C", "pitch", "filter", "rows", "img", "out", "out_bytes", "scratch", "scratch_bytes")]
        return entry(*args) if entry is L.d3ga_png_check else entry(*args, None)
    for entry in (L.d3ga_png_check, L.d3ga_png_encode):
        if entry is L.d3ga_png_check:
            assert status(entry) == OK
        for kw, want in ((dict(C=2), E_CONFIG), (dict(C=0), E_CONFIG), (dict(H=0), E_SIZE), (dict(W=0), E_SIZE), (dict(rows=-1), E_SIZE),
                         (dict(W=2 ** 31 - 1), E_SIZE), (dict(H=2 ** 20, W=2 ** 20, C=1, pitch=2 ** 20, rows=4096), E_SIZE),
                         (dict(pitch=32), E_SIZE), (dict(filter=6), E_CONFIG), (dict(filter=-1), E_CONFIG), (dict(img=None), E_NULL),
                         (dict(out=None), E_NULL), (dict(scratch=None), E_NULL), (dict(out=out + 4), E_CONFIG),
                         (dict(scratch=scr + 8), E_CONFIG), (dict(out_bytes=100), E_CAPACITY), (dict(scratch_bytes=100), E_CAPACITY)):
            assert status(entry, **kw) == want, (kw, want)
    p = R.host_plan(9, 11, 3)
    assert status(L.d3ga_png_check, out_bytes=p["capacity"], scratch_bytes=p["scratch_bytes"]) == OK
    assert status(L.d3ga_png_check, out_bytes=p["capacity"] - 1, scratch_bytes=p["scratch_bytes"]) == E_CAPACITY
    assert L.d3ga_png_capacity(9, 11, 2, 0, None) == E_CONFIG and L.d3ga_png_capacity(0, 11, 3, 0, None) == E_SIZE
    # the Python layer, on a machine without a GPU: nothing is allocated or launched before these raise
    for args in ((0, 4, 3), (4, 0, 3), (4, 4, 2), (4, (2 ** 31 - 1) // 3 + 1, 3), (2 ** 31, 4, 1), (4, 4, 3, -1)):
        with pytest.raises(ValueError, match="PngBuffer: (H|W|C|rows_per_strip)="):
            PngBuffer(*args)
    with pytest.raises(TypeError, match="PngBuffer: H"):
        PngBuffer(4.0, 4, 3)
    with pytest.raises(ValueError, match="img_u8 is on cpu"):
        encode_png(torch.zeros(4, 4, 3, dtype=torch.uint8))
    with pytest.raises(TypeError, match="img_u8 must be uint8"):
        encode_png(torch.zeros(4, 4, 3))
    with pytest.raises(TypeError, match="img_u8"):
        encode_png(np.zeros((4, 4, 3), np.uint8))
