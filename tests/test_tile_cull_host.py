"""Tile lists from the alpha >= 1/255 box (d3ga_raster_params::tile_cull) without a GPU: the rectangle function of d3ga_math.h as a
stand-alone program against a float64 brute force over pixels, and the host layer's switch -- the settings field, its default, the
operators that turn it on and the process-wide override."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT

GROUPS = ("tile_edges", "off_screen", "no_alpha", "between_pixels", "screen_filling", "random")


def test_tight_rectangle_against_float64_brute_force():
    """tests/hostcheck/tile_cull_check.cpp (built as hostcheck.cpp is: g++ -O2 -ffp-contract=off): never larger than the reference
    rectangle, never empty for a visible splat, never without a tile that has an integer pixel inside the box -- on box ends exactly
    on tile edges, centres off-screen, hx = -1, boxes between pixel rows, screen-filling boxes and 60 000 random draws."""
    src = os.path.join(ROOT, "tests", "hostcheck", "tile_cull_check.cpp")
    out_dir = os.path.join(ROOT, "tests", "hostcheck", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "tile_cull_check")
    deps = [src, os.path.join(ROOT, "d3ga_amd", "csrc", "d3ga_math.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr[-3000:])
    lines = out.stdout.strip().splitlines()
    assert [ln.split()[0] for ln in lines] == list(GROUPS), out.stdout
    for ln in lines:
        m = re.fullmatch(r"\w+ cases=(\d+) ok", ln)
        assert m and int(m.group(1)) >= 18, ln
    assert int(re.search(r"cases=(\d+)", lines[-1]).group(1)) > 30000      # (draws whose reference rectangle is empty are skipped)


def test_params_struct_carries_the_field_and_defaults_to_the_reference_rule():
    from d3ga_amd import _lib
    from d3ga_amd import rasterizer as R
    names = [n for n, _ in _lib.RasterParams._fields_]
    assert names[names.index("per_view_geometry") + 1] == "tile_cull" and ctypes.sizeof(_lib.RasterParams) == 4 * len(names)
    # (tests/test_views_appearance_host.py holds the ctypes mirror to the header field by field)
    s = R.GaussianRasterizationSettings(16, 16, 1.0, 1.0, torch.ones(3), 1.0, torch.eye(4), torch.eye(4), 3, torch.zeros(3), False, False)
    assert s.tile_cull is False and s.antialiasing is False
    assert R._params(4, 16, 3, 16, 16, 1.0, 1.0, 1.0, False, False, False, None, False).tile_cull == 0
    on = R._params(4, 16, 3, 16, 16, 1.0, 1.0, 1.0, False, False, False, None, False, tile_cull=True)
    assert on.tile_cull == 1 and on is not R._params(4, 16, 3, 16, 16, 1.0, 1.0, 1.0, False, False, False, None, False)
    assert R._prm_variant(on, acc_self_clearing=1).tile_cull == 1


def test_override_and_the_operators_that_turn_the_rule_on(monkeypatch):
    """renderer.render / render_l1 / render_pair hand the rasterizer settings with tile_cull on; render_views leaves it off unless
    asked; rasterizer.set_tile_cull(True | False) overrides either, None gives the field back its say."""
    from d3ga_amd import rasterizer as R
    from d3ga_amd import renderer
    from d3ga_amd import synthetic as syn
    for requested in (False, True):
        for mode, want in ((None, requested), (True, True), (False, False)):
            R.set_tile_cull(mode)
            try:
                assert R._tile_cull_of(requested) is want
            finally:
                R.set_tile_cull(None)
    with pytest.raises(ValueError):
        R.set_tile_cull("on")
    seen = []

    def recorder(*args, **kw):
        s = args[8]
        seen.append(s.tile_cull)
        img = torch.zeros(3, int(s.image_height), int(s.image_width))
        return img, None, None, img

    for name in ("rasterize_gaussians", "rasterize_gaussians_l1", "rasterize_gaussians_pair"):
        monkeypatch.setattr(renderer, name, recorder)
    batch = syn.make_batch(32, 16, azimuth=0.4)
    pkg = {"means3D": torch.zeros(5, 3), "cov3D_precomp": torch.rand(5, 6), "opacities": torch.rand(5, 1), "shs": torch.rand(5, 16, 3),
           "rgb": None, "sh_degree": 3}
    renderer.render(batch, pkg, torch.ones(3))
    renderer.render_l1(batch, pkg, torch.ones(3), torch.zeros(3, 16, 32))
    renderer.render_pair(batch, pkg, torch.ones(3), torch.rand(5, 3), torch.zeros(3))
    assert seen == [True, True, True]
    import inspect
    from d3ga_amd import raster_views
    assert inspect.signature(renderer.render_views).parameters["tile_cull"].default is False
    assert inspect.signature(raster_views.rasterize_gaussians_views).parameters["tile_cull"].default is False
