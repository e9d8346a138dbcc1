"""Render fusion of the cage deformation's backward (d3ga_amd/cage_deform.py: claim_for_render ... ; csrc/deform_tail.h) without a
GPU: the block merge's index arithmetic as a stand-alone program under the sanitizers, the ABI surface of the new entry points, and
the handshake between a claimed render and the deform node on CPU tensors with the native calls stubbed."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT

NEW_EXPORTS = ("d3ga_raster_preprocess_bwd_deform", "d3ga_raster_backward_deform", "d3ga_raster_backward_l1_deform",
               "d3ga_cage_deform_bwd_tail")


def test_merge_index_arithmetic_under_the_sanitizers(tmp_path):
    """tests/hostcheck/deform_tail_host.cpp: scatter by item_pos and fixed-order segment sums of deform_tail.h against a scalar
    reference, bit for bit, at P = 1, one short of a block, a block, one over, and a partial third block."""
    exe = str(tmp_path / "deform_tail_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "hostcheck", "deform_tail_host.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe, "1", "255", "256", "257", "577"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr[-2000:])
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 5 and all(ln.endswith(" ok") for ln in lines), out.stdout
    assert "blocks=3" in lines[-1]


def test_abi_lists_the_new_entry_points():
    from d3ga_amd import _lib
    from d3ga_amd.csrc import build as b
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "d3ga.h")).read(), flags=re.S)
    L = _lib.lib()
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS and re.search(r"\bint\s+%s\s*\(" % name, src), name
        getattr(L, name)                                   # exported through csrc/d3ga.map (global: d3ga_*)
    assert "global: d3ga_*;" in open(os.path.join(ROOT, "d3ga_amd", "csrc", "d3ga.map")).read()
    assert "deform_tail.h" in b.HEADERS
    assert _lib.ABI_VERSION == 112 and re.search(r"#define\s+D3GA_VERSION\s+112\b", src) and L.d3ga_version() == 112
    # each *_deform entry: its parent's arguments, then the three deform structs, then the stream
    sig = _lib._SIGNATURES
    tail = [ctypes.POINTER(c) for c in (_lib.CageDeformIn, _lib.CageDeformGrads, _lib.CageDeformRoute)]
    for parent in ("d3ga_raster_preprocess_bwd", "d3ga_raster_backward", "d3ga_raster_backward_l1"):
        child = parent + "_deform"
        assert sig[child][0] == sig[parent][0][:-1] + tail + sig[parent][0][-1:] and sig[child][1] is sig[parent][1], child
        proto = lambda n: re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % n, src, re.S).group(1)
        assert len(proto(child).split(",")) == len(proto(parent).split(",")) + 3
    assert sig["d3ga_cage_deform_bwd_tail"] == sig["d3ga_cage_deform_bwd"]
    # refusals that need no GPU: no deform structs; a batch of views
    prm = _lib.RasterParams(P=4, M=16, sh_degree=3, W=16, H=16, tanfovx=1.0, tanfovy=1.0, scale_modifier=1.0)
    none = [None] * 18
    assert L.d3ga_raster_preprocess_bwd_deform(ctypes.byref(prm), *none, None, None, None, None) == -1
    din, dgr = _lib.CageDeformIn(P=4, V=4), _lib.CageDeformGrads()
    prm2 = _lib.RasterParams(P=4, M=16, sh_degree=3, W=16, H=16, tanfovx=1.0, tanfovy=1.0, scale_modifier=1.0, n_views=2)
    assert L.d3ga_raster_preprocess_bwd_deform(ctypes.byref(prm2), *none, ctypes.byref(din), ctypes.byref(dgr), None, None) in (-1, -3)
    din.flags = 8
    assert L.d3ga_raster_preprocess_bwd_deform(ctypes.byref(prm), *none, ctypes.byref(din), ctypes.byref(dgr), None, None) == -3


# ------------------------------------------------------------------------------------------------------------
# the handshake, native calls stubbed
# ------------------------------------------------------------------------------------------------------------
class _FakeLib:
    """Every entry returns D3GA_OK and is recorded; the deform backward fills its per-Gaussian outputs with 2 (CPU memory)."""

    def __init__(self):
        self.calls = []
        self.fail = None

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append(name)
            if name == self.fail:
                return -3
            if name == "d3ga_cage_deform_bwd":
                st, gr = args[0]._obj, args[1]._obj
                for ptr, c in ((gr.g_barys, 4), (gr.g_scales, 3), (gr.g_rots, 4)):
                    if ptr:
                        buf = (ctypes.c_float * (st.P * c)).from_address(ptr)
                        buf[:] = [2.0] * (st.P * c)
            return 0
        return entry

    def d3ga_status_string(self, status):
        return b"stub"


@pytest.fixture
def stub(monkeypatch):
    from d3ga_amd import cage_deform as cd
    fake = _FakeLib()
    monkeypatch.setattr(cd._lib, "lib", lambda: fake)
    monkeypatch.setattr(cd, "require_cuda", lambda *t: None)
    monkeypatch.setattr(cd, "stream_handle", lambda: None)
    cd.set_render_fusion(True)
    yield fake
    cd.set_render_fusion(True)


class _ToyRender(torch.autograd.Function):
    """What the rasterizer's operator does with a claimed node: the fused structs, the deposit (filled with 1), no gradient for the two
    tensors -- or, without a live claim, ordinary gradients."""

    @staticmethod
    def forward(ctx, means, cov6, claim):
        ctx.claim, ctx.shapes = claim, (means.shape, cov6.shape)
        return means.new_zeros(()) + 0.0 * (means.sum() + cov6.sum())

    @staticmethod
    def backward(ctx, g):
        from d3ga_amd import cage_deform as cd
        if ctx.claim is not None and cd.holds_claim(*ctx.claim):
            st, grads, route, dep = cd.fused_tail_structs(ctx.claim[0])
            for k in ("barys", "scales", "rotations", "records"):
                if dep[k] is not None:
                    dep[k].fill_(1.0)
            cd.deposit_on(ctx.claim[0], dep)
            return None, None, None
        return torch.full(ctx.shapes[0], 5.0), torch.full(ctx.shapes[1], 5.0), None


def _inputs(P=5, V=6, T=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    leaf = lambda *s: torch.randn(*s, generator=g).requires_grad_(True)
    tetras = torch.tensor([[0, 1, 2, 3], [1, 2, 3, 4], [2, 3, 4, 5]], dtype=torch.int32)
    tid = torch.randint(0, T, (P,), generator=g).to(torch.int32)
    return dict(tp=leaf(V, 3), tetras=tetras, tid=tid, barys=leaf(P, 4), cg=torch.randn(P, 3, 3, generator=g), scales=leaf(P, 3),
                rots=leaf(P, 4))


def _deform(x):
    from d3ga_amd.cage_deform import cage_deform
    return cage_deform(x["tp"], x["tetras"], x["tid"], x["barys"], x["cg"], x["scales"], x["rots"])


def test_engine_calls_a_node_whose_incoming_gradients_are_all_undefined():
    """What the fused-tail path rests on: no hidden output is needed to keep the deform node in the backward pass."""
    calls = []

    class A(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            ctx.set_materialize_grads(False)
            return x * 2, x * 3

        @staticmethod
        def backward(ctx, g0, g1):
            calls.append((g0, g1))
            return torch.ones(3)

    class B(torch.autograd.Function):
        @staticmethod
        def forward(ctx, a, b, c):
            return (a + b).sum() + c.sum()

        @staticmethod
        def backward(ctx, g):
            return None, None, torch.ones(3) * g
    x, c = torch.zeros(3, requires_grad=True), torch.zeros(3, requires_grad=True)
    B.apply(*A.apply(x), c).backward()
    assert calls == [(None, None)] and torch.equal(x.grad, torch.ones(3))


def test_claim_rules(stub):
    from d3ga_amd import cage_deform as cd
    m, c = _deform(_inputs())
    node, token = cd.claim_for_render(m, c)
    assert node is m.grad_fn and cd.holds_claim(node, token)
    assert cd.claim_for_render(m, c) == (None, None) and not cd.holds_claim(node, token)       # a second render revokes the first
    assert cd.claim_for_render(m, c) == (None, None)
    m, c = _deform(_inputs())
    assert cd.claim_for_render(c, m) == (None, None)                                            # outputs 0 and 1, in this order
    assert cd.claim_for_render(m, c.detach()) == (None, None) and cd.claim_for_render(m.detach(), c) == (None, None)
    assert cd.claim_for_render(m * 1.0, c) == (None, None)                                      # another node's tensor
    with torch.no_grad():
        assert cd.claim_for_render(m, c) == (None, None)
    cd.set_render_fusion(False)
    assert cd.claim_for_render(m, c) == (None, None)
    cd.set_render_fusion(True)
    node, token = cd.claim_for_render(m, c)                                                      # none of the refusals above claimed it
    assert node is not None
    cd.release_claim(node, token)
    assert node.claimed is False
    m.retain_grad()
    assert cd.claim_for_render(m, c) == (None, None)
    m, c = _deform(_inputs())
    c.register_hook(lambda g: g)
    assert cd.claim_for_render(m, c) == (None, None)


def _run(stub, second_consumer=False, claim=True):
    from d3ga_amd import cage_deform as cd
    x = _inputs()
    m, c = _deform(x)
    stub.calls.clear()
    loss = _ToyRender.apply(m, c, cd.claim_for_render(m, c) if claim else None)
    if second_consumer:
        loss = loss + m.sum()
    loss.backward()
    return x, m.grad_fn, [n for n in stub.calls if "cage_deform_bwd" in n]


def test_fused_tail_path(stub):
    from d3ga_amd import cage_deform as cd
    x, node, calls = _run(stub)
    assert calls == ["d3ga_cage_deform_bwd_tail"] and cd.last_backward_path() == "fused-tail"
    assert torch.equal(x["barys"].grad, torch.ones(5, 4)) and torch.equal(x["scales"].grad, torch.ones(5, 3))      # the deposit itself
    assert x["tp"].grad is not None
    assert node.deposit is None and node.claimed is False


def test_kernel_path_without_a_claim(stub):
    from d3ga_amd import cage_deform as cd
    x, node, calls = _run(stub, claim=False)
    assert calls == ["d3ga_cage_deform_bwd"] and cd.last_backward_path() == "kernel"
    assert torch.equal(x["barys"].grad, torch.full((5, 4), 2.0))
    assert node.deposit is None and node.claimed is False


def test_kernel_plus_deposit_path(stub):
    from d3ga_amd import cage_deform as cd
    x, node, calls = _run(stub, second_consumer=True)
    assert calls == ["d3ga_cage_deform_bwd", "d3ga_cage_deform_bwd_tail"] and cd.last_backward_path() == "kernel+deposit"
    assert torch.equal(x["barys"].grad, torch.full((5, 4), 3.0)) and torch.equal(x["rots"].grad, torch.full((5, 4), 3.0))   # kernel 2 + deposit 1
    assert node.deposit is None and node.claimed is False


def test_binding_is_demoted_after_kernel_plus_deposit(stub):
    from d3ga_amd import cage_deform as cd
    x, node, calls = _run(stub, second_consumer=True)
    assert cd.last_backward_path() == "kernel+deposit"
    m, c = _deform(x)                                    # the same binding (tetra_id storage): not claimed again ...
    assert cd.claim_for_render(m, c) == (None, None)
    cd.set_render_fusion(True)                           # ... until re-armed
    assert cd.claim_for_render(m, c)[0] is m.grad_fn


def test_deposit_and_claim_are_cleared_after_an_exception(stub):
    from d3ga_amd import cage_deform as cd
    x = _inputs()
    m, c = _deform(x)
    loss = _ToyRender.apply(m, c, cd.claim_for_render(m, c))
    stub.fail = "d3ga_cage_deform_bwd_tail"
    with pytest.raises(Exception):
        loss.backward(retain_graph=True)
    node = m.grad_fn
    assert node.deposit is None and node.claimed is False
    stub.fail = None


def test_revoked_claim_takes_the_two_kernel_path(stub):
    from d3ga_amd import cage_deform as cd
    x = _inputs()
    m, c = _deform(x)
    first = _ToyRender.apply(m, c, cd.claim_for_render(m, c))
    second = _ToyRender.apply(m, c, cd.claim_for_render(m, c) if cd.claim_for_render(m, c)[0] is not None else None)
    stub.calls.clear()
    (first + second).backward()
    assert [n for n in stub.calls if "cage_deform_bwd" in n] == ["d3ga_cage_deform_bwd"] and cd.last_backward_path() == "kernel"
    assert m.grad_fn.claimed is False


def test_retain_grad_or_hook_between_render_and_backward_ends_the_claim(stub):
    from d3ga_amd import cage_deform as cd
    for late in ("retain_grad", "hook"):
        x = _inputs()
        m, c = _deform(x)
        seen = []
        loss = _ToyRender.apply(m, c, cd.claim_for_render(m, c))
        if late == "retain_grad":
            m.retain_grad()
        else:
            c.register_hook(lambda g: seen.append(g) or g)
        stub.calls.clear()
        loss.backward()
        assert [n for n in stub.calls if "cage_deform_bwd" in n] == ["d3ga_cage_deform_bwd"] and cd.last_backward_path() == "kernel"
        assert (torch.equal(m.grad, torch.full((5, 3), 5.0)) if late == "retain_grad" else len(seen) == 1)
        assert m.grad_fn.claimed is False


def test_the_node_never_references_its_own_outputs(stub):
    """(a cycle tensor -> grad_fn -> tensor through the autograd graph is invisible to the garbage collector)"""
    import weakref
    from d3ga_amd import cage_deform as cd
    m, c = _deform(_inputs())
    node, token = cd.claim_for_render(m, c)
    assert node.claimed is token.key and token.tensors == (m, c)
    alive = weakref.ref(node)
    del m, c, node, token
    assert alive() is None


# the claim rules that live in renderer.render and in the rasterizer's operator, with the rasterizer's native calls stubbed as well
@pytest.fixture
def raster_stub(stub, monkeypatch):
    from d3ga_amd import rasterizer as R
    monkeypatch.setattr(R._lib, "lib", lambda: stub)
    monkeypatch.setattr(R, "require_cuda", lambda *t: None)
    monkeypatch.setattr(R, "stream_handle", lambda: None)
    monkeypatch.setattr(R, "_scratch", lambda *a, **k: [torch.zeros(64, dtype=torch.uint8) for _ in range(3)])
    R.set_capacity_policy("static", 64)
    yield stub
    R.set_capacity_policy("auto")


def _batch(W=16, H=16):
    from d3ga_amd import synthetic as syn
    return syn.make_batch(W, H, azimuth=0.4)


def _pkg(m, c, P=5):
    return {"means3D": m, "cov3D_precomp": c, "opacities": torch.rand(P, 1), "shs": torch.rand(P, 16, 3, requires_grad=True), "rgb": None,
            "sh_degree": 3}


def test_render_claims_and_its_backward_deposits(raster_stub):
    from d3ga_amd import cage_deform as cd
    from d3ga_amd.renderer import render
    x = _inputs()
    m, c = _deform(x)
    img = render(_batch(), _pkg(m, c), torch.ones(3))["render"]
    node = m.grad_fn
    assert node.claimed not in (False, cd._REVOKED)
    raster_stub.calls.clear()
    img.sum().backward()
    assert "d3ga_raster_backward_deform" in raster_stub.calls and "d3ga_raster_backward" not in raster_stub.calls
    assert [n for n in raster_stub.calls if "cage_deform_bwd" in n] == ["d3ga_cage_deform_bwd_tail"]
    assert node.claimed is False and node.deposit is None


def test_render_does_not_claim_with_grad_sync_a_window_or_without_gradients(raster_stub):
    from d3ga_amd.renderer import render

    class Sync:
        world, always, scale = 1, False, 1.0

    x = _inputs()
    m, c = _deform(x)
    render(_batch(), _pkg(m, c), torch.ones(3), grad_sync=Sync())
    assert m.grad_fn.claimed is False                      # render() does not ask with a grad_sync
    from d3ga_amd import synthetic as syn
    from d3ga_amd.cameras import is_cropped
    cropped = syn.make_batch(161, 143, azimuth=0.4, cx=57, cy=96)
    assert is_cropped(cropped)
    render(cropped, _pkg(m, c), torch.ones(3), crop_window=True)
    assert m.grad_fn.claimed is False                      # ... nor for a crop window
    render(_batch(), _pkg(m, c), torch.ones(3))
    assert m.grad_fn.claimed is not False                  # (the plain render of the same package still can)


def test_operator_gives_back_a_claim_it_cannot_serve(raster_stub):
    """_RasterizeGaussians.forward: a windowed camera row, an admitted grad_sync, or a forward without gradients to form releases the
    claim the caller made (release_claim), so a later render of the package can still claim the node."""
    from d3ga_amd import _lib
    from d3ga_amd import cage_deform as cd
    from d3ga_amd import rasterizer as R

    class Sync:
        world, always, scale = 2, True, 1.0

        def verify_inputs(self, inputs):
            pass

    def settings(windowed=False):
        w = _lib.CAMERA_SLOT_WINDOWED
        return R.GaussianRasterizationSettings(16, 16, w if windowed else 1.0, w if windowed else 1.0, torch.ones(3), 1.0, torch.eye(4),
                                               torch.eye(4), 3, torch.zeros(9 if windowed else 3), False, False)
    x = _inputs()
    m, c = _deform(x)
    op, sh = torch.rand(5, 1), torch.rand(5, 16, 3)
    for kw in (dict(s=settings(True)), dict(s=settings(), grad_sync=Sync())):
        claim = cd.claim_for_render(m, c)
        assert claim[0] is not None
        R.rasterize_gaussians(m, None, sh, None, op, None, None, c, kw["s"], kw.get("grad_sync"), deform_node=claim)
        assert m.grad_fn.claimed is False, kw
    claim = cd.claim_for_render(m, c)                      # nothing requires a gradient: forward_only
    R.rasterize_gaussians(m.detach(), None, sh, None, op, None, None, c.detach(), settings(), deform_node=claim)
    assert m.grad_fn.claimed is False
