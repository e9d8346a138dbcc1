"""CPU-side checks of per-view appearance and backgrounds for view-batched rendering (include/d3ga.h:
d3ga_raster_params::per_view_appearance, ::per_view_background): the ctypes mirror of the parameter block follows the header
field by field, the ABI number moved with it, and the shape rules of the Python layer refuse what the kernels cannot take."""
import os
import re

import pytest
import torch

from conftest import ROOT


def _header_fields():
    src = open(os.path.join(ROOT, "include", "d3ga.h")).read()
    body = re.search(r"typedef struct d3ga_raster_params \{(.*?)\} d3ga_raster_params;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(?:int32_t|float)\s+(.*)$", decl, re.S)
        assert m, decl
        names += [n.strip() for n in m.group(1).split(",")]
    return names


def test_raster_params_mirror_the_header_in_order():
    from d3ga_amd._lib import RasterParams
    names = _header_fields()
    assert [f for f, _ in RasterParams._fields_] == names
    assert names[-2:] == ["per_view_appearance", "per_view_background"]
    assert names[-3] == "factor_rows"


def test_abi_version_is_112():
    from d3ga_amd._lib import ABI_VERSION
    assert ABI_VERSION == 112
    ver = int(re.search(r"#define\s+D3GA_VERSION\s+(\d+)", open(os.path.join(ROOT, "include", "d3ga.h")).read()).group(1))
    assert ver == 112


def test_appearance_and_background_shape_rules():
    from d3ga_amd.raster_views import _appearance_per_view, _background_per_view
    k, P = 3, 7
    z = torch.zeros
    assert _appearance_per_view(z(P, 1), z(P, 3), None, k, P) is False
    assert _appearance_per_view(z(P), None, z(P, 16, 3), k, P) is False
    assert _appearance_per_view(z(k, P, 1), z(k, P, 3), None, k, P) is True
    assert _appearance_per_view(z(k, P), z(k, P, 3), None, k, P) is True
    for op, col, sh in ((z(k + 1, P, 1), z(k, P, 3), None),        # a leading dimension that is not k
                        (z(k, P, 1), z(k - 1, P, 3), None),
                        (z(k, P, 1), None, z(P, 16, 3)),           # SH colours with per-view opacities
                        (z(k, P, 1), z(P, 3), None),               # one of the two per view, the other not
                        (z(k, P, 2), z(k, P, 3), None)):
        with pytest.raises(ValueError):
            _appearance_per_view(op, col, sh, k, P)
    assert _background_per_view(z(3), k) is False
    assert _background_per_view(z(k, 3), k) is True
    for bad in (z(k + 1, 3), z(k, 4), z(2 * k)):
        with pytest.raises(ValueError):
            _background_per_view(bad, k)


def test_render_views_refuses_frames_with_different_sh_degrees():
    """the degree was silently taken from the first package."""
    from d3ga_amd.renderer import render_views
    P = 5
    pk = lambda deg: {"means3D": torch.zeros(P, 3), "cov3D_precomp": torch.zeros(P, 6), "opacities": op, "shs": sh, "rgb": None,
                      "sh_degree": deg}
    op, sh = torch.zeros(P, 1), torch.zeros(P, 16, 3)
    with pytest.raises(ValueError, match="sh_degree"):
        render_views(None, [pk(3), pk(2)], torch.ones(3))
    other = dict(pk(3), shs=torch.zeros(P, 16, 3))
    with pytest.raises(ValueError, match="shs"):
        render_views(None, [pk(3), other], torch.ones(3))
