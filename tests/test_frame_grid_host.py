"""The frame grid (d3ga_amd/frame_grid.py) without a GPU: the g++ build of csrc/frame_grid_math.h -- the text
the kernels run -- against torch's and numpy's own quantisers, Python's own number format and an independent numpy restatement
of layout, coverage and blend; the font table; the Python layer's descriptors against brute force; every refusal."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import frame_grid_ref as R
from conftest import ROOT

NEW_EXPORTS = ("d3ga_frame_grid_check", "d3ga_frame_grid")


@pytest.fixture(scope="module")
def font():
    return R.host_font()


def _neighbours(v, n=8):
    """v and its n float32 neighbours on each side"""
    out = [v]
    lo = hi = v
    for _ in range(n):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        out += [lo, hi]
    return out


def _quant_inputs():
    rng = np.random.default_rng(7)
    vals = []
    for k in range(256):
        vals += _neighbours(np.float32(k) / np.float32(255))
        vals += _neighbours(np.float32((k + 0.5) / 255.0))           # where save_image's + 0.5 decides
    tiny = np.float32(1e-45)
    vals += [-tiny, tiny, np.float32(1e-40), np.float32(-1e-40), np.float32(1.1754944e-38), np.float32(-0.0), np.float32(0.0)]
    vals += [np.float32(v) for v in (-1.0, -0.25, -1e-3, 1.0001, 1.5, 2.0, 255.0, 1e10, -1e10, 3e38, -3e38)]
    x = np.concatenate([np.array(vals, np.float32), rng.uniform(-0.5, 1.5, 100000).astype(np.float32)])
    return x


def test_quantisers_equal_torch_and_numpy_bit_for_bit():
    x = _quant_inputs()
    want = R.torch_save_image_u8(torch.from_numpy(x)).numpy()
    got = R.host_quant("save_image", x)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]
    want = R.numpy_clip_u8(x)
    got = R.host_quant("clip", x)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]
    # the two rules differ (so the tests above tell them apart), and what torch / numpy leave undefined is 0 here
    assert (R.host_quant("save_image", x) != R.host_quant("clip", x)).any()
    special = np.array([np.nan, -np.nan, np.inf, -np.inf], np.float32)
    assert R.host_quant("save_image", special).tolist() == [0, 0, 255, 0] and R.host_quant("clip", special).tolist() == [0, 0, 255, 0]


def test_number_format_equals_python():
    fixed = [0.0625, 0.1875, -0.0625, 2.0625, 0.0005, 0.0015, 0.0025, -0.0005,            # ties (the first four are exact)
             9.9995, 0.9996, 99.99951, 999.9995, 99999.9996, -9.9995,                     # carries
             0.0, -0.0, float("inf"), float("-inf"), float("nan"), 1e-45, -1e-45, 1.0, -1.0, 12.3456, 31.415926, 999999.9375, -999999.9375,
             0.001, 0.0004999, 123456.789]
    rng = np.random.default_rng(11)
    rand = np.concatenate([rng.uniform(-1e6, 1e6, 5000), rng.uniform(-100, 100, 3000), rng.uniform(-1, 1, 2000)]).astype(np.float32)
    rand = rand[np.abs(rand) < 1e6]
    assert rand.size >= 9990
    ties = (np.round(rng.uniform(-4000, 4000, 500)) * 2 + 1) / 2000.0          # k.5 / 1000 before the float32 rounding
    for x in fixed + rand.tolist() + ties.tolist():
        x32 = np.float32(x)
        want = f"{float(x32):.3f}"
        assert R.host_format(x32) == want, (x, R.host_format(x32), want)
    assert R.host_format(np.float32(-0.0)) == "-0.000" and R.host_format(np.float32(np.nan)) == "nan"
    assert R.host_format(np.float32(0.0625)) == "0.062" and R.host_format(np.float32(0.1875)) == "0.188"
    # outside the stated domain: the clamped value
    assert R.host_format(np.float32(2e6)) == "999999.999" and R.host_format(np.float32(-1e30)) == "-999999.999"
    assert R.host_format(np.float32(1e6)) == "999999.999" and R.py_format(1e6) == "999999.999"


def test_font_table(font):
    assert font.shape == (95, 7)
    assert (font < 32).all()                                                   # every row inside five columns
    assert not font[0].any()                                                   # the space
    assert all(font[g].any() for g in range(1, 95))
    assert len({font[g].tobytes() for g in range(95)}) == 95
    # a digit, a capital and a punctuation mark reach the cap line and the baseline; a full stop stays at the bottom
    for ch in "0A(":
        g = font[ord(ch) - 32]
        assert g[0] and g[6], ch
    assert not font[ord(".") - 32][:5].any()
    src = open(os.path.join(ROOT, "d3ga_amd", "csrc", "frame_grid_font.h")).read()
    assert len(re.findall(r"^\s*\{0b[01]{5}(?:, 0b[01]{5}){6}\},", src, flags=re.M)) == 95
    code = re.sub(r"//.*", "", src)
    assert "(" not in code.split("kFgFont", 1)[1]                              # data only: a table, no function


@pytest.mark.parametrize("w", [64, 373, 747, 1022, 1920])
def test_layout_rule(w):
    L = R.lib()
    u = L.hc_grid_unit(w)
    assert np.float32(u) == R.unit(w) and u < 17.7
    assert 25 * 6 * float(u) <= w < 26 * 6 * float(u)
    up = float(np.nextafter(np.float32(u), np.float32(np.inf)))
    assert 25 * 6 * up > w                                                     # the largest such float32
    for h in (40, 373, 1080):
        assert L.hc_grid_baseline(u, h, 0) == int(np.float32(10) * np.float32(u)) == R.baseline(np.float32(u), h, False)
        assert L.hc_grid_baseline(u, h, 1) == h - int(np.float32(5) * np.float32(u)) == R.baseline(np.float32(u), h, True)


def test_layout_rule_bound_and_every_width():
    L = R.lib()
    assert np.float32(L.hc_grid_unit(2656)) == np.float32(17.7) and np.float32(L.hc_grid_unit(5000)) == np.float32(17.7)
    assert np.float32(L.hc_grid_unit(2654)) < np.float32(17.7)
    for w in range(1, 2700):
        u = L.hc_grid_unit(w)
        assert np.float32(u) == R.unit(w) and 150.0 * float(u) <= w and u > 0, w


CASES = [("Prediction", 373, 40, False, 2, None), ("Input: Cage", 747, 90, False, 1, None), ("{:.3f} (dB)", 200, 31, True, 2, 31.0625),
         ("3D Means qjy|_", 1022, 120, True, 2, None), ("Wg", 64, 9, False, 2, None), ("~{:.3f}#", 150, 20, False, 1, -0.0)]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_coverage_and_blend_against_the_float64_restatement(font, case):
    """The bound is derived, not measured: coverage within 3 * 2^-24, a blended pixel within 6 * 2^-24."""
    label, w, h, bottom, thickness, value = CASES[case]
    got = R.host_alpha(label, w, h, value=value, bottom=bottom, thickness=thickness)
    want = R.coverage64(R.expand(label, value), w, h, font, bottom=bottom, bold=thickness >= 2)
    err = np.abs(got.astype(np.float64) - want).max()
    print(f"coverage: max |header - float64| = {err / 2.0 ** -24:.3f} x 2^-24")
    assert err <= R.ALPHA_BOUND
    assert got.min() >= 0.0 and got.max() <= 1.0 and (got.max() > 0.5 or w == 64)
    # blend: inputs and colour in [0, 1]
    rng = np.random.default_rng(case)
    img = torch.from_numpy(rng.uniform(0, 1, (3, h, w)).astype(np.float32))
    colour = tuple(float(np.float32(c)) for c in rng.uniform(0, 1, 3))
    cell = None if value is None else torch.tensor([value], dtype=torch.float32)
    out = R.host_write_text(img, label, color=colour, bottom=bottom, thickness=thickness, value=cell).numpy()
    for c in range(3):
        ref = R.blend64(img[c].numpy(), want, colour[c])
        err = np.abs(out[c].astype(np.float64) - ref).max()
        assert err <= R.BLEND_BOUND, (c, err / 2.0 ** -24)
    # a pixel the text does not reach keeps its bits
    assert np.array_equal(out[:, got == 0], img.numpy()[:, got == 0])


def test_text_stays_in_its_box(font):
    w, h = 373, 64
    u = float(R.unit(w))
    base = R.baseline(np.float32(u), h, False)
    a = R.host_alpha("Prediction", w, h)
    ys, xs = np.nonzero(a)
    assert ys.min() >= base - 7 * u - u and ys.max() <= base + u
    assert xs.min() >= 15 - u and xs.max() <= 15 + 6 * u * 10 + u
    thin = R.host_alpha("Prediction", w, h, thickness=1)
    assert (a >= thin).all() and (a > thin).any()                              # bold is a superset
    assert not R.host_alpha("", w, h).any()
    assert np.array_equal(R.host_alpha("\xe9", w, h), R.host_alpha("??", w, h))    # two UTF-8 bytes, two question marks
    assert np.array_equal(R.host_alpha(b"a\x00\x7f", w, h), R.host_alpha("a??", w, h))
    assert R.host_alpha("M" * 64, w, h)[:, -3:].any()                           # wider than the panel: drawn up to its edge
    assert np.array_equal(R.host_alpha("{:.3f} (dB)", w, h, value=9.9995), R.host_alpha(f"{float(np.float32(9.9995)):.3f} (dB)", w, h))


def _views():
    """the same picture as a CHW tensor, an HWC tensor, a transposed view and a channel slice of a wider tensor"""
    g = torch.Generator().manual_seed(3)
    base = torch.rand(3, 9, 13, generator=g)
    hwc = base.permute(1, 2, 0).contiguous()
    transposed = base.permute(0, 2, 1).contiguous().permute(0, 2, 1)           # (3, 9, 13) with the column stride the larger
    wide = torch.rand(6, 9, 13, generator=g)
    wide[1:4] = base
    return base, hwc, transposed, wide[1:4]


def test_descriptor_packing_against_brute_force():
    from d3ga_amd.frame_grid import Panel
    base, hwc, transposed, sliced = _views()
    assert not transposed.is_contiguous() and sliced.storage_offset() > 0
    grey = torch.rand(9, 5, generator=torch.Generator().manual_seed(4))
    rgba = torch.rand(4, 9, 8, generator=torch.Generator().manual_seed(5))
    rows = [[Panel(base), Panel(hwc, layout="hwc"), Panel(grey)], [Panel(transposed), Panel(sliced), Panel(rgba[:3, :, :5])]]
    got = R.host_compose_rows(rows, quantize=None)
    top = torch.cat([base, base, grey[None].expand(3, -1, -1)], dim=2)
    bot = torch.cat([base, base, rgba[:3, :, :5]], dim=2)
    want = torch.nn.functional.pad(torch.cat([top, bot], dim=1), (0, 1, 0, 0), value=1.0)      # 31 wide -> 32; 18 high stays
    assert got.shape == (3, 18, 32) and np.array_equal(got, want.numpy())
    # HWC float output, four channels (alpha 1 where the source has none), BGR
    got = R.host_compose_rows(rows, quantize=None, out_layout="hwc", channels=4, order="bgr", pad_value=0.25)
    want4 = torch.cat([torch.nn.functional.pad(torch.cat([top, bot], dim=1), (0, 1, 0, 0), value=0.25).flip(0),
                       torch.ones(1, 18, 32)], dim=0)
    want4[3, :, 31] = 0.25
    assert np.array_equal(got, want4.permute(1, 2, 0).numpy())
    # uint8 with a padded pitch; the RGBA panel's own alpha
    out, _ = R.host_compose([(Panel(rgba), 0, 0)], (9, 8), quantize="clip", channels=4, pitch=40)
    assert np.array_equal(out, R.numpy_clip_u8(rgba.permute(1, 2, 0).numpy()))


def _desc(n=1, **kw):
    """a valid one-launch table over addresses that are never read"""
    from d3ga_amd import _lib
    d = _lib.GridDesc()
    d.n_panels, d.out_H, d.out_W, d.mode, d.channels, d.pad_value, d.pitch = n, 8, 16 * n, _lib.GRID_OUT_U8_SAVE_IMAGE, 3, 1.0, 48 * n
    for i in range(n):
        e = d.panel[i]
        e.src, e.sc, e.sh, e.sw, e.C, e.h, e.w, e.y0, e.x0, e.X = 4096, 128, 16, 1, 3, 8, 16, 0, 16 * i, 15
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _check(d, out=8192):
    from d3ga_amd import _lib
    path = ctypes.c_int32(-1)
    st = _lib.lib().d3ga_frame_grid_check(ctypes.byref(d), ctypes.c_void_p(out), ctypes.byref(path))
    return st, path.value


def test_path_decision_and_c_abi_refusals():
    from d3ga_amd import _lib
    assert _check(_desc(2)) == (0, 1)
    assert _check(_desc(16)) == (0, 1)
    for field, value in (("src", 4100), ("x0", 1), ("sw", 3), ("sh", 18), ("sc", 130), ("w", 15)):
        d = _desc(1, out_W=20, pitch=60)                     # room for the panel one column to the right
        assert _check(d) == (0, 1)
        setattr(d.panel[0], field, value)
        assert _check(d) == (0, 0), field
    assert _check(_desc(1, pitch=49)) == (0, 0) and _check(_desc(1), out=8194) == (0, 0)
    assert _check(_desc(1, out_W=18, pitch=54)) == (0, 0)
    assert _check(_desc(1, flags=_lib.GRID_FORCE_SCALAR)) == (0, 0)
    assert _check(_desc(1, mode=_lib.GRID_OUT_F32_CHW), out=8192) == (0, 1) and _check(_desc(1, mode=_lib.GRID_OUT_F32_CHW), out=8196) == (0, 0)
    d = _desc(1)
    d.panel[0].C, d.panel[0].sc = 1, 3                      # a one-channel source never reads sc
    assert _check(d) == (0, 1)
    # refusals: the same statuses as everywhere in the library
    assert _check(_desc(1, n_panels=17))[0] == -2 and _check(_desc(1, n_panels=0))[0] == -2
    assert _check(_desc(1, out_H=0))[0] == -2 and _check(_desc(1, out_W=_lib.GRID_MAX_SIDE + 1))[0] == -2
    assert _check(_desc(1, mode=4))[0] == -3 and _check(_desc(1, channels=5))[0] == -3 and _check(_desc(1, flags=4))[0] == -3
    assert _check(_desc(1, pitch=47))[0] == -2
    assert _check(_desc(1), out=0)[0] == -1
    for field, value, status in (("src", 0, -1), ("C", 2, -3), ("h", 0, -2), ("h", 9, -2), ("x0", 4, -2), ("y0", -1, -2), ("sw", -1, -2),
                                 ("label_len", 65, -2), ("label_len", -1, -2), ("flags", 4, -3), ("value", 4096, -3)):
        d = _desc(1)
        setattr(d.panel[0], field, value)
        assert _check(d)[0] == status, (field, value)
    d = _desc(2)
    d.panel[1].x0 = 12                                       # shares four columns with panel 0
    d.out_W = 32
    assert _check(d)[0] == -3
    d = _desc(1)
    d.panel[0].label, d.panel[0].label_len = b"{:.3f} and {:.3f}", 17
    d.panel[0].value = 4096
    assert _check(d)[0] == -3
    d.panel[0].label_len = 6
    assert _check(d)[0] == 0
    d.panel[0].value = None                                  # a slot without its cell
    assert _check(d)[0] == -3
    # the launch entry refuses the same before it launches anything
    assert _lib.lib().d3ga_frame_grid(ctypes.byref(_desc(1, n_panels=17)), ctypes.c_void_p(8192), None, None) == -2
    assert _lib.lib().d3ga_frame_grid(None, ctypes.c_void_p(8192), None, None) == -1


def test_plan_matches_the_restatement():
    from d3ga_amd.frame_grid import Panel, _pack
    from d3ga_amd import _lib
    panels = [Panel(torch.zeros(3, 20, 373), "a {:.3f} b", value=torch.zeros(1), bottom=True), Panel(torch.zeros(3, 20, 64), "plain")]
    d = _pack([(panels[0], 0, 0), (panels[1], 0, 373)], 20, 437, _lib.GRID_OUT_F32_CHW, 3, "rgb", 1.0, 0)
    unit, base, slot, path = (ctypes.c_float * 16)(), (ctypes.c_int32 * 16)(), (ctypes.c_int32 * 16)(), ctypes.c_int32()
    assert R.lib().hc_grid_plan(ctypes.byref(d), ctypes.c_void_p(64), ctypes.byref(path), unit, base, slot) == 0
    assert [np.float32(unit[i]) for i in range(2)] == [R.unit(373), R.unit(64)]
    assert list(base[:2]) == [R.baseline(R.unit(373), 20, True), R.baseline(R.unit(64), 20, False)] and list(slot[:2]) == [2, -1]
    buf = ctypes.create_string_buffer(96)
    keep = (ctypes.c_float * 1)(-12.3456)
    d.panel[0].value = ctypes.addressof(keep)
    n = R.lib().hc_grid_label(ctypes.byref(d), ctypes.c_void_p(64), buf)
    assert buf.raw[:n] == b"a -12.346 b" == R.expand("a {:.3f} b", -12.3456)


def test_python_layer_refusals():
    from d3ga_amd import D3GAError
    from d3ga_amd.frame_grid import GridWriter, Panel, compose_grid, compose_panels, to_uint8, write_text
    img = torch.zeros(3, 8, 16)
    with pytest.raises(ValueError, match=r"17 panels"):
        compose_grid([[Panel(img)] * 17])
    with pytest.raises(ValueError, match="65 bytes"):
        Panel(img, "x" * 65)
    with pytest.raises(ValueError, match="65 bytes"):
        Panel(img, "x" * 63 + "\xe9")                        # 64 characters, 65 bytes
    Panel(img, "x" * 64)
    with pytest.raises(ValueError, match="at most one"):
        Panel(img, "{:.3f} / {:.3f}", value=torch.zeros(1))
    with pytest.raises(ValueError, match="do not fit"):
        Panel(img, "{:.3f}")
    with pytest.raises(ValueError, match="do not fit"):
        Panel(img, "no slot", value=torch.zeros(1))
    with pytest.raises(ValueError, match="overlap"):
        compose_panels([(Panel(img), 0, 0), (Panel(img), 4, 8)], (16, 32))
    with pytest.raises(ValueError, match="leaves the canvas"):
        compose_panels([(Panel(img), 0, 4)], (8, 16))
    with pytest.raises(D3GAError, match="GPU only"):
        compose_grid([[Panel(img)]])
    with pytest.raises(D3GAError, match="GPU only"):
        to_uint8(img)
    with pytest.raises(D3GAError, match="GPU only"):
        write_text(img, "label")
    for bad in (torch.float16, torch.float64, torch.uint8):
        with pytest.raises(TypeError, match="float32"):
            Panel(img.to(bad))
        with pytest.raises(TypeError, match="float32"):
            Panel(img, "{:.3f}", value=torch.zeros(1).to(bad))
    with pytest.raises(TypeError, match="compose_grid"):
        write_text(np.zeros((8, 16, 3), np.float32), "label")
    with pytest.raises(TypeError, match="compose_grid"):
        Panel(np.zeros((3, 8, 16), np.float32))
    with pytest.raises(ValueError, match="2 channels"):
        Panel(torch.zeros(2, 8, 16))
    with pytest.raises(ValueError, match=r"row 0 entry 1 .* 9 rows high"):
        compose_grid([[Panel(img), Panel(torch.zeros(3, 9, 16), "tall")]])
    with pytest.raises(ValueError, match=r"row 1 .*'wide'.* is 17 pixels wide, row 0 is 16"):
        compose_grid([[Panel(img)], [Panel(torch.zeros(3, 8, 17), "wide")]])
    with pytest.raises(ValueError, match="quantize"):
        compose_grid([[Panel(img)]], quantize="round")
    with pytest.raises(ValueError, match="order"):
        compose_grid([[Panel(img)]], order="grb")
    with pytest.raises(ValueError, match="channels"):
        compose_grid([[Panel(img)]], channels=1)
    with pytest.raises(TypeError, match="uint8"):
        GridWriter(2).submit(torch.zeros(4, 4))
    with pytest.raises(D3GAError, match="GPU only"):
        GridWriter(2).submit(torch.zeros(4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="depth"):
        GridWriter(0)


def test_abi_lists_the_new_entry_points():
    import d3ga_amd
    from d3ga_amd import _lib, frame_grid
    from d3ga_amd.csrc import build as b
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "d3ga.h")).read(), flags=re.S)
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS and re.search(r"\bint\s+%s\s*\(" % name, src), name
    assert "frame_grid.hip" in b.SOURCES and "frame_grid_math.h" in b.HEADERS and "frame_grid_font.h" in b.HEADERS
    assert "-ffp-contract=off" in b.EXTRA["frame_grid.hip"]
    assert [len(_lib._SIGNATURES[n][0]) for n in NEW_EXPORTS] == [3, 4]
    assert _lib.ABI_VERSION == 112 and re.search(r"#define\s+D3GA_VERSION\s+112\b", src) and _lib.lib().d3ga_version() == 112
    for n in ("GRID_MAX_PANELS", "GRID_MAX_LABEL", "GRID_MAX_SIDE", "GRID_OUT_F32_CHW", "GRID_OUT_F32_HWC", "GRID_OUT_U8_SAVE_IMAGE",
              "GRID_OUT_U8_CLIP", "GRID_BGR", "GRID_FORCE_SCALAR", "PANEL_BOTTOM", "PANEL_BOLD"):
        assert getattr(_lib, n) == int(re.search(r"#define\s+D3GA_%s\s+(\d+)" % n, src).group(1)), n
    assert ctypes.sizeof(_lib.GridPanel) == 152 and ctypes.sizeof(_lib.GridDesc) == 40 + 16 * 152
    assert frame_grid.MAX_PANELS == 16 and frame_grid.MAX_LABEL == 64
    for n in ("Panel", "compose_grid", "to_uint8", "write_text", "GridWriter"):
        assert n in d3ga_amd.__all__ and getattr(d3ga_amd, n) is getattr(frame_grid, n)
