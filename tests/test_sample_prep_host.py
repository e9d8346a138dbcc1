"""Sample preparation without a GPU: the numpy oracle (tests/sample_prep_ref.py) against the reference's own loader lines
(tests/golden/sample_prep_cases.npz, tools/gen_sample_prep_golden.py) and against torch's F.interpolate; the g++ build of
csrc/sample_prep_math.h -- the text the kernels run -- against the oracle, byte for byte, on both store paths; the fixed cases of
the rules; the ABI surface and its refusals; the Python layer's ValueErrors.  Everything is integer or exactly representable:
every comparison is equality."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sample_prep_ref as sr
from conftest import ROOT

E_NULL, E_SIZE, E_CONFIG = -1, -2, -3            # D3GA_E_* (include/d3ga.h)
SIZES = [(1, 1), (1, 5), (3, 1), (2, 3), (5, 7), (16, 64), (17, 63), (33, 65), (9, 260)]
GOLIATH_SIZES = [(2, 2), (7, 9), (64, 48), (5, 4), (3, 16), (9, 260)]


def _equal(got, want, what):
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k], want[k]), (what, k)


def test_oracle_equals_the_reference_loader(golden):
    z = golden("sample_prep_cases.npz")
    assert [str(n) for n in z["names"]] == ["a", "b", "c"]
    for n in ("a", "b", "c"):
        image, seg, alpha = z[f"{n}_image_bgr"], z[f"{n}_seg_bgr"], z[f"{n}_alpha_bgr"]
        H, W = image.shape[:2]
        assert 36 <= H <= 44 and 44 <= W <= 52 and alpha.shape == (H, W, 3) and seg.shape[0] >= H and seg.shape[1] >= W
        m = alpha[..., 0]
        assert {0, 5, 6, 127, 128, 129, 249, 250, 255} <= set(m.ravel().tolist())
        want = sr.actorshq_ref(image[None], seg[None], m[None], np.float32)
        assert np.array_equal(want["image"][0], z[f"{n}_image"]) and z[f"{n}_image"].dtype == np.float32
        assert np.array_equal(want["seg_part"][0], z[f"{n}_seg_part"]) and z[f"{n}_seg_part"].dtype == np.int32
        assert set(z[f"{n}_seg_part"].ravel().tolist()) == {0, 1, 2, 3, 4}
        # the loader hands out bool planes; Batcher.process makes float32 of them (lib/batch.py:151-152)
        assert np.array_equal(want["seg_fg"][0], z[f"{n}_seg_fg"].astype(np.float32))
        assert np.array_equal(want["boundary_fg"][0], z[f"{n}_boundary_fg"].astype(np.float32))
        b, f = sr.boundary_and_fg(m)                          # get_boundary_mask called on its own
        assert np.array_equal(b, z[f"{n}_mask_boundary"]) and np.array_equal(f, z[f"{n}_mask_fg"])
        assert 0.2 < b.mean() < 0.9 and 0.2 < f.mean() < 0.8
    assert z["a_seg_bgr"].shape[:2] == (42, 53)               # larger than the image by (2, 5)


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("B", [1, 3])
def test_host_build_equals_the_oracle(H, W, B):
    image, seg, mask = sr.random_actorshq(H * 1000 + W + B, B, H, W, extra=(2, 5))
    for dtype in (np.uint8, np.float32):
        want = sr.actorshq_ref(image, seg, mask, dtype)
        got, path = sr.host_actorshq(image, seg, mask, dtype)
        assert path == int(W % 4 == 0)
        _equal(got, want, ("planned", dtype))
        got, path = sr.host_actorshq(image, seg, mask, dtype, force_scalar=True)
        assert path == 0
        _equal(got, want, ("scalar", dtype))
    # the matte as channel 0 of (B,H,W,3); a row-padded image; the part image cropped out of a larger buffer
    matte = np.random.default_rng(1).integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    matte[..., 0] = mask
    padded = np.full((B, H, W + 3, 3), 0xAB, np.uint8)
    padded[:, :, :W] = image
    big = np.full((B, H + 4, W + 9, 3), 0xCD, np.uint8)
    big[:, :H + 2, :W + 5] = seg
    got, _ = sr.host_actorshq(padded[:, :, :W], big[:, :H + 2, :W + 5], matte[..., 0])
    _equal(got, sr.actorshq_ref(image, seg, mask), "views")
    skipped, _ = sr.host_actorshq(image, seg, mask, skip=("image", "seg_fg"))
    assert skipped["image"] is None and skipped["seg_fg"] is None
    assert np.array_equal(skipped["seg_part"], got["seg_part"]) and np.array_equal(skipped["boundary_fg"], got["boundary_fg"])


def _interpolate(x):
    return F.interpolate(torch.from_numpy(x).float(), scale_factor=0.5, mode="bilinear").numpy()


@pytest.mark.parametrize("H,W", GOLIATH_SIZES)
def test_goliath_oracle_and_host_build_equal_interpolate_bit_for_bit(H, W):
    for B in (1, 2):
        image, parts = sr.random_goliath(H * 100 + W + B, B, H, W)
        image[0, :, :2, :2] = 255                             # the largest mean
        want = sr.goliath_ref(image, parts)
        fg = _interpolate((parts != 0).astype(np.uint8))
        torch_says = {"image": _interpolate(image), "seg_part": _interpolate(parts), "seg_fg": fg, "boundary_fg": 1 - fg}
        _equal(want, torch_says, "oracle against F.interpolate")
        assert want["image"].shape == (B, 3, H // 2, W // 2) and want["image"].max() == 255.0
        got, path = sr.host_goliath(image, parts)
        assert path == int((W // 2) % 4 == 0)
        _equal(got, want, "host build")
        assert np.array_equal(got["seg_part"].astype(np.int32), np.trunc(want["seg_part"]).astype(np.int32))     # what .int() makes of it
    skipped, _ = sr.host_goliath(image, parts, skip=("image", "boundary_fg"))
    assert np.array_equal(skipped["seg_fg"], want["seg_fg"]) and skipped["image"] is None


def _one(mask, seg=None):
    """one frame through the g++ build AND the oracle (they must agree) -> (label, fg, boundary) as (H,W) arrays"""
    mask = np.asarray(mask, np.uint8)
    H, W = mask.shape
    seg = np.zeros((H, W, 3), np.uint8) if seg is None else np.asarray(seg, np.uint8)
    image = np.zeros((H, W, 3), np.uint8)
    got, _ = sr.host_actorshq(image[None], seg[None], mask[None], force_scalar=True)
    _equal(got, sr.actorshq_ref(image[None], seg[None], mask[None]), "fixed case")
    if W % 4 == 0:
        _equal(sr.host_actorshq(image[None], seg[None], mask[None])[0], got, "fixed case, four pixels per thread")
    return got["seg_part"][0, 0], got["seg_fg"][0, 0], got["boundary_fg"][0, 0]


def test_fixed_cases_of_the_matte_rules():
    # a uniform matte: the window is flat, so boundary is the soft-value rule alone and fg is m > 128
    for m, fg, boundary in ((0, 0, 0), (5, 0, 0), (6, 0, 1), (127, 0, 1), (128, 0, 1), (129, 1, 1), (249, 1, 1), (250, 1, 0), (255, 1, 0)):
        _, f, b = _one(np.full((5, 8), m))
        assert (f == fg).all() and (b == boundary).all(), m
    # a 128 inside a window of ones: t = 128 there, di - er = 127 around it -> no edge; of zeros: 128, no edge either
    for around in (255, 0):
        m = np.full((5, 5), around)
        m[2, 2] = 128
        _, f, b = _one(m)
        want_b = np.zeros((5, 5))
        want_b[2, 2] = 1                                      # by 5 < 128 < 250 alone
        assert np.array_equal(b, want_b) and f[2, 2] == 0 and (f[m == 255] == 1).all()
    # an edge between 0 and 255 marks both sides, one pixel deep; a 128 next to the edge hides the 1 - 0 step from its neighbours
    m = np.zeros((4, 8))
    m[:, 4:] = 255
    _, f, b = _one(m)
    assert np.array_equal(b, np.tile([0, 0, 0, 1, 1, 0, 0, 0], (4, 1))) and np.array_equal(f, m == 255)
    m[1, 4] = 128
    _, f, b = _one(m)
    assert b[1, 4] == 1 and b[0, 3] == 0 and b[1, 3] == 0 and b[2, 3] == 0 and b[3, 3] == 1 and b[3, 4] == 1
    assert b[0, 5] == 0 and b[2, 5] == 0 and b[1, 5] == 0


@pytest.mark.parametrize("y,x", [(0, 0), (0, 3), (0, 7), (2, 0), (2, 7), (4, 0), (4, 3), (4, 7)], ids=lambda v: str(v))
def test_window_is_clipped_at_each_border_and_corner(y, x):
    """One background pixel on the border of a foreground image: erosion must see only the in-image part of the window (a border
    that counted as 0 would mark the whole frame's rim), dilation must not pick anything up from outside."""
    m = np.full((5, 8), 255)
    _, f, b = _one(m)
    assert not b.any() and f.all()                            # nothing outside leaks in, on any border
    m[y, x] = 0
    _, f, b = _one(m)
    yy, xx = np.mgrid[0:5, 0:8]
    assert np.array_equal(b, (abs(yy - y) <= 1) & (abs(xx - x) <= 1)) and f[y, x] == 0


def test_images_smaller_than_the_window():
    for shape in ((1, 1), (1, 2), (2, 1), (2, 2)):
        m = np.full(shape, 255)
        assert not _one(m)[2].any()
        m[0, 0] = 0
        assert _one(m)[2].all() == (shape != (1, 1))          # a single pixel is its whole window: no step to see


def test_fixed_cases_of_the_label_rule():
    colours = {  # (r, g, b) -> label
        (255, 0, 0): 1, (0, 255, 0): 2, (0, 0, 255): 3, (127, 127, 127): 4,
        (127, 0, 0): 4, (127, 9, 200): 4,                    # a native red of 127 is gray
        (0, 0, 0): 4,                                        # foreground without a colour: taken as 127s
        (255, 255, 0): 2, (255, 0, 255): 3, (0, 255, 255): 3, (255, 255, 255): 3,     # two or three channels claim it: the later wins
        (127, 255, 255): 4, (127, 255, 0): 4,
        (0, 127, 0): 0, (0, 0, 127): 0, (254, 1, 128): 0, (1, 0, 0): 0, (126, 126, 126): 0,
    }
    rgb = np.array(list(colours), np.uint8)
    seg = np.ascontiguousarray(rgb[None, :, ::-1])            # (1, n, 3) BGR
    n = len(colours)
    label, f, _ = _one(np.full((1, n), 255), seg)
    assert label[0].tolist() == list(colours.values()) and f.all()
    for m in (0, 127, 128):                                   # no foreground (128 stays 128, not 1): label 0 whatever the colour
        label, f, _ = _one(np.full((1, n), m), seg)
        assert not label.any() and not f.any(), m
    label, _, _ = _one(np.full((1, n), 129), seg)
    assert label[0].tolist() == list(colours.values())


def _tensors(B=2, H=6, W=8, extra=(1, 2)):
    image, seg, mask = sr.random_actorshq(3, B, H, W, extra)
    return torch.from_numpy(image), torch.from_numpy(seg), torch.from_numpy(mask)


def test_python_layer_validates_on_the_host():
    from d3ga_amd import _lib
    from d3ga_amd.sample_prep import prepare_actorshq, prepare_goliath
    B, H, W = 2, 6, 8
    img, seg, mask = _tensors(B, H, W)
    matte = torch.zeros(B, H, W, 3, dtype=torch.uint8)
    wide = torch.zeros(B, H, W, 4, dtype=torch.uint8)
    f32 = lambda *s: torch.zeros(*s)
    bad = [
        lambda: prepare_actorshq(img.numpy(), seg, mask),                                      # not a tensor
        lambda: prepare_actorshq(img[..., :2], seg, mask),                                     # not (..., 3)
        lambda: prepare_actorshq(img.permute(0, 3, 1, 2), seg, mask),                          # planar: not (B,H,W,3)
        lambda: prepare_actorshq(img.float(), seg, mask),                                      # dtype
        lambda: prepare_actorshq(img, seg.int(), mask),
        lambda: prepare_actorshq(img, seg, mask.bool()),
        lambda: prepare_actorshq(img, seg[:, : H - 1], mask),                                  # Hs < H
        lambda: prepare_actorshq(img, seg[:, :, : W - 1], mask),                               # Ws < W
        lambda: prepare_actorshq(img, seg[:1], mask),                                          # another B
        lambda: prepare_actorshq(img, seg, mask[:, :, :-1]),                                   # mask shape
        lambda: prepare_actorshq(img[0], seg, mask[0]),                                        # 3-D and 4-D mixed
        lambda: prepare_actorshq(torch.zeros(B, H, W, 6, dtype=torch.uint8)[..., ::2], seg, mask),     # channels two bytes apart
        lambda: prepare_actorshq(wide[..., :3], seg, mask),                                    # pixels 4 bytes apart
        lambda: prepare_actorshq(img, torch.zeros(B, H + 1, W + 2, 6, dtype=torch.uint8)[..., :3], mask),     # seg pixels 6 bytes apart
        lambda: prepare_actorshq(img, seg, wide[..., 0]),                                      # mask pixels 4 bytes apart
        lambda: prepare_actorshq(img, seg, mask.transpose(1, 2).contiguous().transpose(1, 2)),  # column-major mask
        lambda: prepare_actorshq(img[:1].expand(B, H, W, 3), seg, mask),                       # frames overlap
        lambda: prepare_actorshq(img, seg, mask, image_dtype=torch.float16),
        lambda: prepare_actorshq(img, seg, mask, out={"alpha": f32(B, 1, H, W)}),              # unknown slot
        lambda: prepare_actorshq(img, seg, mask, out={"seg_part": f32(B, 1, H, W)}),           # int32 wanted
        lambda: prepare_actorshq(img, seg, mask, out={"seg_fg": f32(B, 1, H, W + 1)}),
        lambda: prepare_actorshq(img, seg, mask, out={"image": torch.zeros(B, 3, H, W, dtype=torch.float64)}),
        lambda: prepare_actorshq(img, seg, mask, out={"boundary_fg": f32(B, 1, W, H).transpose(2, 3)}),
        lambda: prepare_actorshq(img, seg, mask, out={"seg_fg": torch.zeros(B * H * W + 1)[1:].view(B, 1, H, W)}),     # alignment
        lambda: prepare_actorshq(img, seg, mask, out={"seg_fg": torch.zeros(B, 1, H, W, device="meta")}),
    ]
    gimg, gparts = torch.zeros(B, 3, H, W, dtype=torch.uint8), torch.zeros(B, 1, H, W, dtype=torch.uint8)
    bad += [
        lambda: prepare_goliath(gimg[:, :2], gparts),
        lambda: prepare_goliath(gimg.float(), gparts),
        lambda: prepare_goliath(gimg, gparts.int()),
        lambda: prepare_goliath(gimg, gparts[:, :, :-1]),
        lambda: prepare_goliath(gimg[:, :, :1], gparts[:, :, :1]),                             # H < 2
        lambda: prepare_goliath(gimg[..., :1], gparts[..., :1]),                               # W < 2
        lambda: prepare_goliath(gimg[..., ::2], gparts[..., ::2]),                             # elements of a row two bytes apart
        lambda: prepare_goliath(gimg[:, :1].expand(B, 3, H, W), gparts),                       # channels overlap
        lambda: prepare_goliath(gimg[0], gparts),                                              # 3-D and 4-D mixed
        lambda: prepare_goliath(gimg, gparts, out={"image": f32(B, 3, H, W)}),                 # full size: H // 2 wanted
        lambda: prepare_goliath(gimg, gparts, out={"seg_part": torch.zeros(B, 1, H // 2, W // 2, dtype=torch.int32)}),
    ]
    for i, fn in enumerate(bad):
        with pytest.raises(ValueError):
            fn()
            pytest.fail(f"case {i} was accepted")
    # everything fits -- views included -- but the tensors live on the CPU: no fallback
    for fn in (lambda: prepare_actorshq(img, seg, mask), lambda: prepare_actorshq(img[0], seg[0], matte[0]),
               lambda: prepare_actorshq(img[:, 1:, 2:], seg[:, :, 1:], matte[:, 1:, 2:]), lambda: prepare_goliath(gimg, gparts),
               lambda: prepare_goliath(gimg[0, :, 1:, 1:], gparts[0, :, 1:, 1:])):
        with pytest.raises(_lib.D3GAError):
            fn()


def test_sample_prep_owns_a_frame_prep():
    from d3ga_amd.frame_prep import FramePrep
    from d3ga_amd.sample_prep import SamplePrep
    cages = {"body": {"label_id": [1]}, "upper": {"label_id": [2]}, "lower": {"label_id": [3]}}
    p = SamplePrep({"train": {"erode_mask": True, "use_gamma_space": True, "background": "Black"}, "cages": cages})
    assert isinstance(p.frame_prep, FramePrep) and (p.frame_prep.erode_mask, p.frame_prep.gamma, p.frame_prep.background) == (True, True, "black")
    img, seg, mask = _tensors()
    with pytest.raises(ValueError):
        p.actorshq(img, seg, mask, out={"render": torch.zeros(1)})
    with pytest.raises(ValueError):
        p.goliath(torch.zeros(1, 3, 4, 4, dtype=torch.uint8), torch.zeros(1, 1, 4, 4, dtype=torch.uint8), out={"parts": torch.zeros(1)})


def test_new_abi_surface():
    from d3ga_amd import _lib
    src = open(os.path.join(ROOT, "include", "d3ga.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], capture_output=True, text=True, check=True).stdout
    for name, n_args in (("d3ga_sample_prep_actorshq", 22), ("d3ga_sample_prep_goliath", 16)):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
        assert re.search(r"\bint\s+%s\s*\(" % name, src)
        assert re.search(r"\bT %s$" % name, out, flags=re.M)                     # through csrc/d3ga.map
        assert len(_lib._SIGNATURES[name][0]) == n_args
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, src).group(1)
        assert decl.count(",") + 1 == n_args
    assert "d3ga_*" in open(os.path.join(ROOT, "d3ga_amd", "csrc", "d3ga.map")).read()
    assert _lib.ABI_VERSION == 112 and re.search(r"#define\s+D3GA_VERSION\s+112\b", src) and _lib.lib().d3ga_version() == 112
    build = open(os.path.join(ROOT, "d3ga_amd", "csrc", "build.py")).read()
    assert "sample_prep.hip" in build and "sample_prep_math.h" in build
    import d3ga_amd
    assert d3ga_amd.SamplePrep and d3ga_amd.prepare_actorshq and d3ga_amd.prepare_goliath


def _buffers():
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    return buf, p, ctypes.c_void_p(p.value + 4), ctypes.c_void_p(p.value + 1)


@pytest.mark.parametrize("which", ["library", "host build"])
def test_actorshq_entry_point_refuses_bad_arguments_before_any_launch(which):
    """The refusals happen before any HIP call: host buffers stand in for device memory and are never touched.  The g++ build runs
    the same plan function and must give the same statuses."""
    from d3ga_amd import _lib
    buf, p, off4, off1 = _buffers()
    path = ctypes.c_int32(-5)
    H, W, Hs, Ws = 4, 8, 5, 10
    ok = dict(B=2, H=H, W=W, Hs=Hs, Ws=Ws, image=p, image_pitch=3 * W, image_frame=3 * W * H, seg=p, seg_pitch=3 * Ws, seg_frame=3 * Ws * Hs,
              mask=p, mask_pitch=W, mask_frame=W * H, mask_step=1, image_f32=0, image_out=p, seg_part_out=p, seg_fg_out=p, boundary_out=p)
    if which == "library":
        call = lambda **kw: _lib.lib().d3ga_sample_prep_actorshq(*{**ok, **kw}.values(), ctypes.byref(path), None)
    else:
        call = lambda **kw: sr.lib().hc_sample_prep_actorshq(*{**ok, **kw}.values(), ctypes.byref(path), 0)
    for name in ("B", "H", "W", "Hs", "Ws"):
        assert call(**{name: 0}) == E_SIZE and call(**{name: -2}) == E_SIZE, name
    assert call(B=65536) == E_SIZE
    big = dict(image_pitch=2 ** 40, seg_pitch=2 ** 40, mask_pitch=2 ** 40, image_frame=2 ** 62, seg_frame=2 ** 62, mask_frame=2 ** 62)
    assert call(H=2 ** 16, W=2 ** 15, Hs=2 ** 16, Ws=2 ** 15, **big) == E_SIZE                  # H W > INT32_MAX
    assert call(H=262141, W=1, Hs=262141, Ws=1, **big) == E_SIZE                               # more rows than the grid has
    assert call(Hs=H - 1) == E_SIZE and call(Ws=W - 1) == E_SIZE
    assert call(image_pitch=3 * W - 1) == E_CONFIG and call(seg_pitch=3 * Ws - 1) == E_CONFIG and call(mask_pitch=W - 1) == E_CONFIG
    assert call(mask_step=3) == E_CONFIG                      # the row is (W - 1) 3 + 1 bytes long then
    assert call(image_frame=3 * W * H - 1) == E_CONFIG and call(seg_frame=3 * Ws * H - 1) == E_CONFIG and call(mask_frame=W * H - 1) == E_CONFIG
    for step in (0, 2, 4, -1):
        assert call(mask_step=step) == E_CONFIG, step
    assert call(image_f32=2) == E_CONFIG and call(image_f32=-1) == E_CONFIG
    for name in ("image", "seg", "mask"):
        assert call(**{name: None}) == E_NULL, name
    assert call(image_out=None, seg_part_out=None, seg_fg_out=None, boundary_out=None) == E_NULL
    for name in ("seg_part_out", "seg_fg_out", "boundary_out"):
        assert call(**{name: off4}) == E_CONFIG, name
    assert call(image_out=off4, image_f32=1) == E_CONFIG
    assert path.value == -5 and not any(buf)
    if which == "host build":                                 # what is accepted, and the path it takes (host memory: only here)
        small = dict(B=1, H=2, W=8, Hs=2, Ws=8, seg_pitch=24)
        assert call(**small) == 0 and path.value == 1
        assert call(image_out=off4, **small) == 0 and path.value == 1         # a uint8 image needs 4 bytes for the four-pixel path
        assert call(image_out=off1, **small) == 0 and path.value == 0
        assert call(**{**small, "W": 7, "image_pitch": 21}) == 0 and path.value == 0
        assert call(B=1, H=1, W=3, Hs=1, Ws=3, image_pitch=9, seg_pitch=9, mask_pitch=7, mask_step=3, image_frame=0, seg_frame=0, mask_frame=0) == 0


@pytest.mark.parametrize("which", ["library", "host build"])
def test_goliath_entry_point_refuses_bad_arguments_before_any_launch(which):
    from d3ga_amd import _lib
    buf, p, off4, _ = _buffers()
    path = ctypes.c_int32(-5)
    H, W = 4, 6
    ok = dict(B=2, H=H, W=W, image=p, image_pitch=W, image_plane=W * H, image_frame=3 * W * H, parts=p, parts_pitch=W, parts_frame=W * H,
              image_out=p, seg_part_out=p, seg_fg_out=p, boundary_out=p)
    if which == "library":
        call = lambda **kw: _lib.lib().d3ga_sample_prep_goliath(*{**ok, **kw}.values(), ctypes.byref(path), None)
    else:
        call = lambda **kw: sr.lib().hc_sample_prep_goliath(*{**ok, **kw}.values(), ctypes.byref(path))
    assert call(B=0) == E_SIZE and call(B=-1) == E_SIZE and call(B=65536) == E_SIZE
    for name in ("H", "W"):
        for v in (1, 0, -3):
            assert call(**{name: v}) == E_SIZE, (name, v)
    big = dict(image_pitch=2 ** 40, parts_pitch=2 ** 40, image_plane=2 ** 59, image_frame=2 ** 62, parts_frame=2 ** 62)
    assert call(H=2 ** 16, W=2 ** 15, **big) == E_SIZE
    assert call(image_pitch=W - 1) == E_CONFIG and call(parts_pitch=W - 1) == E_CONFIG
    assert call(image_plane=W * H - 1) == E_CONFIG and call(image_frame=3 * W * H - 1) == E_CONFIG and call(parts_frame=W * H - 1) == E_CONFIG
    assert call(image=None) == E_NULL and call(parts=None) == E_NULL
    assert call(image_out=None, seg_part_out=None, seg_fg_out=None, boundary_out=None) == E_NULL
    for name in ("image_out", "seg_part_out", "seg_fg_out", "boundary_out"):
        assert call(**{name: off4}) == E_CONFIG, name
    assert path.value == -5 and not any(buf)
    if which == "host build":
        assert call(B=1) == 0 and path.value == 0
        assert call(B=1, H=2, W=9, image_pitch=9, parts_pitch=9, image_plane=18) == 0 and path.value == 1
        assert call(B=1, image_out=None) == 0
