"""The element-wise kernels every field network begins or ends in (csrc/encoding.hip: field_heads, view_dirs, sh4_encoding,
color_rows) against float64 restatements (tests/field_ref.py, oracle.mlp.sh4_direction_encoding) at the places the goldens do
not reach: other head layouts and row counts, saturated activations, unused heads, refused arguments, view directions next to
and far from the camera and along the axes, and empty Gaussian sets."""
import ctypes
import os

import numpy as np
import pytest
import torch

import field_ref
from cage_ref import GuardedBuffer
from conftest import ROOT
from oracle import mlp as om
from util import elementwise_excess, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

LAYOUTS = [[(1, "none", 0.0)],
           [(3, "tanh", 0.07)],
           [(4, "tanh", 1.0), (4, "none", 0.0), (3, "none", 0.0)],
           [(3, "sigmoid", 0.0), (1, "sigmoid", 0.1)],
           [(1, "tanh", -0.5), (1, "sigmoid", -2.0), (1, "none", 0.0), (1, "tanh", 1e-3)],
           [(2, "none", 0.0), (5, "sigmoid", 0.3), (1, "tanh", 2.0), (7, "none", 0.0)],
           [(128, "tanh", 0.3)]]
ROWS = [1, 37, 255, 256, 257, 1000]
# The backward forms the slope from the float32 output y (a - y^2 / a, y (1 - y)): a u-ulp error in y moves it by up to
# 2 u 2^-24 |a| however small the true slope is.  u = 2 for tanhf / expf plus the multiply and the divide, times two, and a
# factor of about 2 of room: 16 x 2^-24 x |a| x |upstream| on top of 1e-5 relative.
C_FLOOR = 16
WORST = {"none": 0.0, "tanh": 0.0, "sigmoid": 0.0}       # the largest share of the allowance any case of this run used


def _width(spec):
    return sum(w for w, _, _ in spec)


def _as_kernel_sees(spec):
    """The spec with every param rounded to float32 (the entry points take float): the reference evaluates the same numbers."""
    return [(w, act, float(np.float32(p))) for w, act, p in spec]


def _device_heads(pred, spec, ups):
    """field_heads on the device from CPU float32 tensors -> (heads, pred.grad), both on the device."""
    from d3ga_amd.mlp import field_heads
    leaf = pred.to(DEV).requires_grad_(True)
    out = field_heads(leaf, spec)
    torch.autograd.backward(out, [u.to(DEV) for u in ups])
    return out, leaf.grad


def _ref_heads(pred, spec, ups):
    """The same in float64 on the same float32 values -> (heads, pred.grad)."""
    leaf = pred.detach().double().requires_grad_(True)
    out = field_ref.heads(leaf, _as_kernel_sees(spec))
    torch.autograd.backward(out, [u.double() for u in ups])
    return [o.detach() for o in out], leaf.grad


def _assert_heads_close(out, ref, spec, P):
    assert len(out) == len(spec)
    for o, r, (w, act, _) in zip(out, ref, spec):
        assert o.shape == (P, w) and o.is_contiguous() and o.dtype == torch.float32, (act, o.shape, o.stride())
        np.testing.assert_allclose(o.detach().cpu().numpy(), r.numpy(), rtol=1e-5, atol=2e-6, err_msg=f"head {act} of width {w}")


def _grad_shares(d, ref, spec, ups):
    """Per activation the worst |d - ref| / (1e-5 |ref| + C_FLOOR 2^-24 s_h |g|), s_h = |param| for tanh and 1 otherwise
    (<= 1 passes), printed and kept in WORST."""
    g = torch.cat([u.double() for u in ups], dim=1).abs()
    s = torch.cat([torch.full((w,), abs(float(np.float32(p))) if act == "tanh" else 1.0, dtype=torch.float64) for w, act, p in spec])
    diff = (d.detach().cpu().double() - ref).abs()
    allow = 1e-5 * ref.abs() + C_FLOOR * 2.0 ** -24 * s * g
    share = torch.where(diff == 0, torch.zeros_like(diff), diff / allow)          # (an upstream of exactly 0 allows nothing but 0)
    assert not torch.isnan(share).any()
    seen, c = {}, 0
    for w, act, _ in spec:
        if share.shape[0]:
            seen[act] = max(seen.get(act, 0.0), float(share[:, c:c + w].max()))
        c += w
    for act, v in seen.items():
        WORST[act] = max(WORST[act], v)
    print(f"[field heads] share of the gradient allowance used: {seen}; worst so far {WORST}")
    return seen


@pytest.mark.parametrize("P", ROWS)
@pytest.mark.parametrize("layout", range(len(LAYOUTS)))
def test_heads_layouts_against_f64(layout, P):
    """field_heads through autograd against float64, over layouts the goldens do not have (one to four heads, widths 1 to 128,
    negative and small tanh factors) and row counts on either side of the 256-thread block.  pred = 4 randn puts a good share
    of the tanh and sigmoid outputs on the flat part, where the backward's slope is a cancellation."""
    spec = LAYOUTS[layout]
    N = _width(spec)
    g = torch.Generator().manual_seed(1000 * layout + P)
    pred = 4.0 * torch.randn(P, N, generator=g)
    ups = [torch.randn(P, w, generator=g) for w, _, _ in spec]
    out, grad = _device_heads(pred, spec, ups)
    ref, ref_grad = _ref_heads(pred, spec, ups)
    _assert_heads_close(out, ref, spec, P)
    assert grad.shape == (P, N) and grad.dtype == torch.float32
    shares = _grad_shares(grad, ref_grad, spec, ups)
    assert max(shares.values()) <= 1.0, shares
    c = 0
    for (w, act, _), u in zip(spec, ups):                    # an identity head hands its upstream through untouched
        if act == "none":
            assert torch.equal(grad[:, c:c + w].cpu(), u)
        c += w


SATURATING = [0.0, 1e-8, 5.0, 9.02, 20.0, 88.0, 89.0, 104.0, 1e4, 3e38]


@pytest.mark.parametrize("spec", [[(3, "sigmoid", 0.0), (1, "sigmoid", 0.1)], [(3, "tanh", 0.07)],
                                  [(3, "tanh", 0.2)], [(4, "tanh", 0.25), (4, "none", 0.0), (3, "none", 0.0)]],
                         ids=["color", "tanh0.07", "deformation", "canonical"])
def test_heads_saturation_is_finite_and_signed(spec):
    """Inputs from +-0 to +-3e38 (tanhf saturates past 9.02, expf under- and overflows around 88 / 104): outputs finite and
    inside the activation's range, gradients finite and never of the sign opposite to the true slope's -- a slope formed from
    the saturated output may round to zero, not through it.  The layouts are ColorField's, the (3, tanh, 0.07) one, and the
    defaults of DeformationField and CanonicalField."""
    P, N = 64, _width(spec)
    vals = torch.tensor([s * v for v in SATURATING for s in (1.0, -1.0)])
    pred = vals[(torch.arange(P)[:, None] + 5 * torch.arange(N)[None, :]) % len(vals)]      # every column meets every value
    g = torch.Generator().manual_seed(N)
    ups = [torch.randn(P, w, generator=g) for w, _, _ in spec]
    out, grad = _device_heads(pred, spec, ups)
    ref, ref_grad = _ref_heads(pred, spec, ups)
    _assert_heads_close(out, ref, spec, P)
    grad, c = grad.cpu(), 0
    assert torch.isfinite(grad).all()
    for o, (w, act, a), u in zip(out, spec, ups):
        o, d = o.detach().cpu(), grad[:, c:c + w]
        assert torch.isfinite(o).all()
        if act == "sigmoid":
            assert float(o.min()) >= 0.0 and float(o.max()) <= 1.0
            assert bool((d * torch.sign(u) >= 0).all()), (act, a, float((d * torch.sign(u)).min()))
        elif act == "tanh":
            assert float(o.abs().max()) <= abs(float(np.float32(a)))
            assert bool((d * torch.sign(a * u) >= 0).all()), (act, a, float((d * torch.sign(a * u)).min()))
        c += w
    shares = _grad_shares(grad, ref_grad, spec, ups)
    assert max(shares.values()) <= 1.0, shares


def test_heads_dtype_and_strided_inputs():
    """A float64 pred, a pred that is a column slice of a wider tensor and upstream gradients with stride 0 (what
    head.sum().backward() hands over) give the contiguous float32 call's values and gradients bit for bit, and pred.grad comes
    back in pred's dtype and shape."""
    from d3ga_amd.mlp import field_heads
    spec, P = LAYOUTS[5], 257
    N = _width(spec)
    g = torch.Generator().manual_seed(3)
    wide = (4.0 * torch.randn(P, N + 9, generator=g)).to(DEV)
    scale = [torch.tensor(0.25 * (h + 1), device=DEV) for h in range(len(spec))]
    base = wide[:, 4:4 + N].contiguous().requires_grad_(True)
    out0 = field_heads(base, spec)
    torch.autograd.backward(out0, [s.expand(P, w).contiguous() for s, (w, _, _) in zip(scale, spec)])
    for name, leaf in (("float64", wide[:, 4:4 + N].double().requires_grad_(True)),
                       ("column slice", wide[:, 4:4 + N].detach().requires_grad_(True))):
        assert name == "float64" or not leaf.is_contiguous()
        out = field_heads(leaf, spec)
        ups = [s.expand(P, w) for s, (w, _, _) in zip(scale, spec)]
        assert all(u.stride() == (0, 0) for u in ups)
        torch.autograd.backward(out, ups)
        for a, b in zip(out, out0):
            assert a.dtype == torch.float32 and a.is_contiguous() and torch.equal(a, b), name
        assert leaf.grad.dtype == leaf.dtype and leaf.grad.shape == leaf.shape, name
        assert torch.equal(leaf.grad, base.grad.to(leaf.dtype)), name


# ---- the C entry points themselves ---------------------------------------------------------------------------------


def _lib_and_codes():
    import d3ga_amd
    with open(os.path.join(ROOT, "include", "d3ga.h")) as f:
        return d3ga_amd.lib(), field_ref.status_codes(f.read())


def _c_spec(spec):
    n = len(spec)
    return (n, (ctypes.c_int32 * n)(*[w for w, _, _ in spec]), (ctypes.c_int32 * n)(*[field_ref.ACT[a] for _, a, _ in spec]),
            (ctypes.c_float * n)(*[p for _, _, p in spec]))


def test_heads_unused_head_has_zero_gradient():
    """d3ga_field_heads_bwd with a NULL g_h ("a head nobody used", which autograd never passes: it materialises gradients):
    that head's columns of d_pred are exactly 0, every other column is what the call with all four gradients gives, and every
    element of d_pred is written."""
    from d3ga_amd._lib import dptr, stream_handle
    L, codes = _lib_and_codes()
    spec, P = LAYOUTS[5], 37
    N = _width(spec)
    g = torch.Generator().manual_seed(5)
    pred = (4.0 * torch.randn(P, N, generator=g)).to(DEV)
    ups = [torch.randn(P, w, generator=g).to(DEV) for w, _, _ in spec]
    out = GuardedBuffer("out", (P * N,), DEV)
    assert L.d3ga_field_heads_fwd(P, N, *_c_spec(spec), dptr(pred), out.ptr(), stream_handle()) == codes["OK"]
    out.check()
    ref, _ = _ref_heads(pred.cpu(), spec, [u.cpu() for u in ups])
    np.testing.assert_allclose(out.t.cpu().numpy(), torch.cat([r.reshape(-1) for r in ref]).numpy(), rtol=1e-5, atol=2e-6)

    def backward(present):
        d = GuardedBuffer("d_pred", (P, N), DEV)
        gs = [dptr(u) if h in present else None for h, u in enumerate(ups)]
        assert L.d3ga_field_heads_bwd(P, N, *_c_spec(spec), out.ptr(), *gs, d.ptr(), stream_handle()) == codes["OK"]
        d.check()
        return d.t.cpu()
    full = backward({0, 1, 2, 3})
    assert all(bool((full[:, c] != 0).any()) for c in range(N))
    start = np.cumsum([0] + [w for w, _, _ in spec])
    for absent in ({0}, {1}, {2}, {3}, {0, 1, 2, 3}):
        d = backward({0, 1, 2, 3} - absent)
        for h in range(4):
            cols = slice(int(start[h]), int(start[h + 1]))
            if h in absent:
                assert float(d[:, cols].abs().max()) == 0.0, (absent, h)
            else:
                assert torch.equal(d[:, cols], full[:, cols]), (absent, h)


def test_heads_refusals_launch_nothing():
    """Every refused argument set of tests/field_ref.py (the table tests/test_abi_and_host.py runs without a device) on real
    buffers: the documented status, and not one element of any output written."""
    L, codes = _lib_and_codes()
    g = torch.Generator().manual_seed(7)
    pred, up = torch.randn(8, 6, generator=g).to(DEV), torch.randn(8, 6, generator=g).to(DEV)
    out, d_pred = GuardedBuffer("out", (48,), DEV), GuardedBuffer("d_pred", (8, 6), DEV)
    field_ref.check_heads_refusals(L, codes, pred.data_ptr(), out.ptr(), up.data_ptr(), d_pred.ptr())
    dirs = torch.nn.functional.normalize(torch.randn(8, 3, generator=g), dim=-1).to(DEV)
    feats = torch.randn(8 * 8 + 1, generator=g).to(DEV)
    x, enc = GuardedBuffer("x", (8 * 24 + 1,), DEV), GuardedBuffer("enc", (8 * 16 + 1,), DEV)
    d_dirs, d_feats = GuardedBuffer("d_dirs", (8, 3), DEV), GuardedBuffer("d_feats", (8 * 8 + 1,), DEV)
    field_ref.check_encoding_refusals(L, codes, dirs.data_ptr(), feats.data_ptr(), x.ptr(), enc.ptr(), d_dirs.ptr(), d_feats.ptr())
    torch.cuda.synchronize()
    for buf in (out, d_pred, x, enc, d_dirs, d_feats):
        buf.untouched()


# ---- view directions and the SH encoding at the edges ----------------------------------------------------------------

DISTANCES = (1e-3, 1.0, 1e3, 1e5)


def _edge_means(cam, seed):
    """257 means around `cam` (float32 arithmetic throughout): per distance 6 axis directions, 8 diagonals and 50 random ones,
    and one more random row at distance 1 -> (means, index into DISTANCES per row, mask of the axis and diagonal rows)."""
    g = torch.Generator().manual_seed(seed)
    axes = torch.cat([torch.eye(3), -torch.eye(3)])
    diag = torch.tensor([[a, b, c] for a in (1.0, -1.0) for b in (1.0, -1.0) for c in (1.0, -1.0)]) / 3.0 ** 0.5
    rand = torch.nn.functional.normalize(torch.randn(50, 3, generator=g), dim=-1)
    dirs = torch.cat([axes, diag, rand])
    means = torch.cat([cam + d * dirs for d in DISTANCES] + [cam + torch.nn.functional.normalize(torch.randn(1, 3, generator=g), dim=-1)])
    group = torch.cat([torch.full((64,), k) for k in range(len(DISTANCES))] + [torch.tensor([1])])
    special = torch.cat([torch.arange(64) < 14] * len(DISTANCES) + [torch.tensor([False])])
    assert means.shape == (257, 3) and float(torch.linalg.norm(means - cam, dim=-1).min()) > 0
    return means, group, special


@pytest.mark.parametrize("cam", [(1000.25, -999.5, 3.0), (0.0, 0.0, 0.0)], ids=["far_camera", "origin"])
def test_view_dirs_near_far_and_axis_aligned(cam):
    """d3ga_view_dirs_* a millimetre from the camera, 100 km from it and in between, in random directions, along the axes
    (where x = 2 v - 1 makes several SH terms vanish) and along the diagonals: values, and the Jacobian (I - v v^T) / |m - c|
    per distance group -- it scales with 1 / |m - c|, so one comparison over all groups would see the nearest only.  The axis and
    diagonal rows then go on into sh4_direction_encoding and into _ColorRows, as in test_view_dirs_and_sh4_encoding_match_oracle."""
    from d3ga_amd.mlp import _ColorRows, sh4_direction_encoding, view_directions
    cam = torch.tensor(cam)
    means, group, special = _edge_means(cam, 21)
    g = torch.Generator().manual_seed(22)
    up = torch.randn(257, 3, generator=g)
    m64 = means.double().requires_grad_(True)
    v64 = field_ref.view_dirs(m64, cam.double())
    v64.backward(up.double())
    md = means.to(DEV).requires_grad_(True)
    v = view_directions(md, cam.to(DEV)[None])
    v.backward(up.to(DEV))
    np.testing.assert_allclose(v.detach().cpu().numpy(), v64.detach().numpy(), rtol=0, atol=2e-7)
    for k, dist in enumerate(DISTANCES):
        rows = group == k
        err = rel_err(md.grad.cpu()[rows].numpy(), m64.grad[rows].numpy())
        print(f"[view dirs] camera {cam.tolist()} distance {dist:g}: gradient rel_err {err:.2e}")
        assert err < 1e-5, (dist, err)
    # the axis and diagonal rows through the encoding, both ways it is reached
    F = 4
    ms, gs = means[special], group[special]
    feats, up_x = torch.randn(len(ms), F, generator=g), torch.randn(len(ms), 16 + F, generator=g)
    m64 = ms.double().requires_grad_(True)
    e64 = om.sh4_direction_encoding(field_ref.view_dirs(m64, cam.double()))
    e64.backward(up_x[:, :16].double())
    m1 = ms.to(DEV).requires_grad_(True)
    e1 = sh4_direction_encoding(view_directions(m1, cam.to(DEV)[None]))
    e1.backward(up_x[:, :16].to(DEV))
    m2, f2 = ms.to(DEV).requires_grad_(True), feats.to(DEV).requires_grad_(True)
    x2 = _ColorRows.apply(view_directions(m2, cam.to(DEV)[None]), f2)
    x2.backward(up_x.to(DEV))
    assert torch.equal(x2[:, 16:].cpu(), feats) and torch.equal(f2.grad.cpu(), up_x[:, 16:])
    for name, e, m in (("sh4_direction_encoding", e1, m1), ("_ColorRows", x2[:, :16], m2)):
        np.testing.assert_allclose(e.detach().cpu().numpy(), e64.detach().numpy(), rtol=1e-5, atol=2e-6, err_msg=name)
        for k, dist in enumerate(DISTANCES):
            rows = gs == k
            excess = elementwise_excess(m.grad.cpu()[rows].numpy(), m64.grad[rows].numpy(), atol_rel=1e-5)
            print(f"[view dirs] camera {cam.tolist()} distance {dist:g} through {name}: excess {excess:.3f}")
            assert excess <= 1.0, (name, dist, excess)


def test_view_dirs_zero_distance_is_contained():
    """A mean that coincides with the camera has no direction (0 / 0, as the reference's own expression): whatever that row
    holds, every other row's value and gradient are those of the run without it, bit for bit."""
    from d3ga_amd.mlp import view_directions
    g = torch.Generator().manual_seed(31)
    cam = torch.tensor([0.3, -0.2, 4.0])
    means, up = torch.randn(300, 3, generator=g) * 2.0, torch.randn(300, 3, generator=g)
    at = 150
    means_z, up_z = torch.cat([means[:at], cam[None], means[at:]]), torch.cat([up[:at], torch.ones(1, 3), up[at:]])

    def run(m, u):
        leaf = m.to(DEV).requires_grad_(True)
        v = view_directions(leaf, cam.to(DEV))
        v.backward(u.to(DEV))
        return v.detach().cpu(), leaf.grad.cpu()
    v, d = run(means, up)
    vz, dz = run(means_z, up_z)
    assert torch.isfinite(v).all() and torch.isfinite(d).all()
    keep = torch.arange(301) != at
    assert torch.equal(vz[keep], v) and torch.equal(dz[keep], d)


# ---- empty sets ----------------------------------------------------------------------------------------------------


def _assert_no_parameter_gradient(module):
    for name, p in module.named_parameters():
        assert p.grad is None or (p.grad.shape == p.shape and not bool(p.grad.any())), name


def test_empty_inputs_give_empty_outputs_and_zero_parameter_gradients():
    """A Gaussian set with no rows (the rasterizer renders an empty scene: test_gpu_views.py, test_gpu_parity.py) goes through
    the glue ops and the field networks: empty float32 outputs of the right widths on the device, a backward that runs, (0, .)
    input gradients, and nothing but zeros in the gradients of the parameters and of the broadcast inputs."""
    from d3ga_amd.mlp import (CanonicalField, ColorField, DeformationField, _ColorRows, field_heads, sh4_direction_encoding,
                              view_directions)
    empty = lambda *w: torch.zeros(0, *w, device=DEV).requires_grad_(True)
    vec = lambda n, seed: torch.randn(n, generator=torch.Generator().manual_seed(seed)).to(DEV).requires_grad_(True)

    def check(outs, widths, row_inputs, broadcast=(), module=None):
        outs = outs if isinstance(outs, (tuple, list)) else (outs,)
        assert [tuple(o.shape) for o in outs] == [(0, w) for w in widths]
        assert all(o.dtype == torch.float32 and o.device == torch.device(DEV) for o in outs)
        sum(o.sum() for o in outs).backward()
        for t in row_inputs:
            assert t.grad is not None and t.grad.shape == t.shape
        for t in broadcast:
            assert t.grad is not None and t.grad.shape == t.shape and not bool(t.grad.any())
        if module is not None:
            _assert_no_parameter_gradient(module)

    m = empty(3)
    check(view_directions(m, torch.tensor([[0.3, -0.2, 4.0]], device=DEV)), [3], [m])
    d = empty(3)
    check(sh4_direction_encoding(d), [16], [d])
    for F in (0, 24):
        d, f = empty(3), empty(F)
        check(_ColorRows.apply(d, f), [16 + F], [d, f])
    pred = empty(15)
    check(field_heads(pred, LAYOUTS[5]), [2, 5, 1, 7], [pred])

    torch.manual_seed(41)
    col = ColorField().to(DEV)                               # the per-row path: [enc | pose | frame | shs]
    shs, pose, vd, frame = empty(64), vec(98, 1), empty(3), vec(32, 2)
    check(col(shs, pose, vd, frame_encoding=frame), [3, 1], [shs, vd], [pose, frame], col)
    col = ColorField(n_features=24, n_cond=30, frame_dims=8, n_nodes=64, n_layers=2, shadow_dims=1).to(DEV)
    shs, pose, vd, frame, shadow = empty(24), vec(30, 3), empty(3), vec(8, 4), empty(1)      # a shadow column: the general path
    check(col(shs, pose, vd, frame_encoding=frame, shadow=shadow), [3, 1], [shs, vd, shadow], [pose, frame], col)
    col = ColorField(n_features=24, n_cond=30, frame_dims=8, camera_dims=6, n_nodes=64, n_layers=2, shadow_dims=1).to(DEV)
    shs, pose, vd, frame, camera, shadow = empty(24), vec(30, 5), empty(3), vec(8, 6), vec(6, 7), empty(1)
    check(col(shs, pose, vd, frame_encoding=frame, camera_encoding=camera, shadow=shadow), [3, 1], [shs, vd, shadow],
          [pose, frame, camera], col)
    can = CanonicalField().to(DEV)
    barys, rots, scales, pose = empty(4), empty(4), empty(3), vec(98, 8)
    check(can(barys, rots, scales, pose), [4, 4, 3], [barys, rots, scales], [pose], can)
    dfm = DeformationField().to(DEV)
    canonical, pose = empty(3), vec(98, 9)
    check(dfm(canonical, pose), [3], [canonical], [pose], dfm)
