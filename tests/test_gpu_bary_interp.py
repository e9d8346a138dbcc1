"""d3ga_bary_interp_{fwd,bwd} and d3ga_amd.bary_interp on the GPU against the float64 restatement of tests/bary_ref.py, within
the derived bars stated there (no outliers, no element left out), at the smallest shapes at which the kernels can go wrong:
P around the workgroup and wavefront sizes, both K, C at both ends and odd, V = 1 (every item on one row: lists of thousands,
across every lane split), V = 5 with one row nobody reads, V = 300 (mostly short and empty lists)."""
import functools
import itertools

import pytest
import torch

import bary_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"

PS, KS, CS, VS = (0, 1, 63, 64, 65, 257, 1000), (3, 4), (1, 3, 8), (1, 5, 300)
# the cross product thinned by a Latin square: every (P, K) meets every C and every V once, every (C, V) pair appears
CASES = [(P, K, CS[t], VS[(t + j) % 3]) for j, (P, K) in enumerate(itertools.product(PS, KS)) for t in range(3)]


@functools.lru_cache(maxsize=None)
def case(P, K, C, V):
    """Seeded inputs on both sides, the binding, and the float64 reference with and without delta_barys: computed once, shared,
    never written to."""
    from d3ga_amd.bary_interp import BaryBinding
    g = torch.Generator().manual_seed(1000 * P + 100 * K + 10 * C + V % 7)
    if V == 5:
        rows = torch.tensor([0, 1, 2, 4])[torch.randint(0, 4, (P, K), generator=g)]          # row 3: an empty list
    else:
        rows = torch.randint(0, V, (P, K), generator=g)
    attr = torch.randn(V, C, generator=g)
    barys = torch.rand(P, K, generator=g)
    barys = barys / barys.sum(1, keepdim=True).clamp_min(1e-3)
    delta = torch.tanh(torch.randn(P, K, generator=g)) * 0.05
    g_out = torch.randn(P, C, generator=g)
    cpu = dict(rows=rows, attr=attr, barys=barys, delta=delta, g_out=g_out)
    dev = {k: v.to(DEV) for k, v in cpu.items()}
    return dict(cpu=cpu, dev=dev, binding=BaryBinding(dev["rows"], n_rows=V),
                ref={True: bary_ref.interp_ref(attr, rows, barys, delta, g_out), False: bary_ref.interp_ref(attr, rows, barys, None, g_out)})


def raw(c, P, K, C, V, with_delta, want_attr=True, want_barys=True):
    """Both entry points on buffers pre-filled with NaN -> (out, g_attr | None, g_barys | None)."""
    from d3ga_amd import _lib
    from d3ga_amd._lib import check, dptr, stream_handle
    d, b = c["dev"], c["binding"]
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)
    out, g_attr, g_barys = nan(P, C), nan(V, C) if want_attr else None, nan(P, K) if want_barys else None
    delta = d["delta"] if with_delta else None
    L = _lib.lib()
    check(L.d3ga_bary_interp_fwd(P, K, C, dptr(d["attr"]), dptr(b.rows), dptr(d["barys"]), dptr(delta), dptr(out), stream_handle()),
          "d3ga_bary_interp_fwd")
    check(L.d3ga_bary_interp_bwd(P, V, K, C, dptr(d["attr"]), dptr(b.rows), dptr(d["barys"]), dptr(delta), dptr(d["g_out"]),
                                 dptr(b.vert_start), dptr(b.vert_items), dptr(g_attr), dptr(g_barys), stream_handle()),
          "d3ga_bary_interp_bwd")
    return out, g_attr, g_barys


@pytest.mark.parametrize("P,K,C,V", CASES)
def test_entry_points_write_every_element_within_the_bars(P, K, C, V):
    c = case(P, K, C, V)
    for with_delta in (True, False):
        ref = c["ref"][with_delta]
        bar = bary_ref.bars(ref, K, C)
        got = dict(zip(("out", "g_attr", "g_barys"), raw(c, P, K, C, V, with_delta)))
        for name in ("out", "g_attr", "g_barys"):
            bary_ref.assert_within(f"P{P} K{K} C{C} V{V} delta={with_delta} {name}", got[name], ref[name], bar[name])
        if P == 0:
            assert not got["g_attr"].any()                                   # every list is empty: exact zeros, written by the call
        elif V == 5 and P >= 63:
            assert not got["g_attr"][3].any() and got["g_attr"][0].any()     # the row nobody reads
        again = raw(c, P, K, C, V, with_delta)
        for name, t in zip(("out", "g_attr", "g_barys"), again):
            assert torch.equal(t, got[name]), name                           # fixed summation order: bit-identical
    # each gradient alone is the same launch with the other skipped
    only_attr, only_barys = raw(c, P, K, C, V, True, want_barys=False), raw(c, P, K, C, V, True, want_attr=False)
    both = raw(c, P, K, C, V, True)
    assert only_attr[2] is None and torch.equal(only_attr[1], both[1])
    assert only_barys[1] is None and torch.equal(only_barys[2], both[2])


def test_lists_cross_every_lane_split():
    """The shapes above hold what the issue asks for: one row's list longer than 64 and than 256 items, empty lists, V = 1."""
    lens = {(P, K, C, V): case(P, K, C, V)["ref"][True]["L"] for (P, K, C, V) in CASES if P >= 257}
    assert any(V == 1 and l.max() > 256 for (P, K, C, V), l in lens.items())
    assert any(V == 5 and l.max() > 256 and l.min() == 0 for (P, K, C, V), l in lens.items())
    assert any(V == 300 and 0 < l.max() < 64 and l.min() == 0 for (P, K, C, V), l in lens.items())
    assert any(64 < l.max() <= 256 for l in lens.values())
    assert {(C, V) for (_, _, C, V) in CASES} == set(itertools.product(CS, VS))


def leaves(c, delta=True, req=(True, True, True)):
    d = c["dev"]
    attr, barys = d["attr"].clone().requires_grad_(req[0]), d["barys"].clone().requires_grad_(req[1])
    dl = d["delta"].clone().requires_grad_(req[2]) if delta else None
    return attr, barys, dl


@pytest.mark.parametrize("K", KS)
def test_autograd_path_equals_the_entry_points_bit_for_bit(K):
    from d3ga_amd.bary_interp import bary_interp
    P, C, V = 257, 3, 300
    c = case(P, K, C, V)
    for with_delta in (True, False):
        attr, barys, dl = leaves(c, with_delta)
        out = bary_interp(attr, c["binding"], barys, dl)
        out.backward(c["dev"]["g_out"])
        r_out, r_ga, r_gb = raw(c, P, K, C, V, with_delta)
        assert torch.equal(out, r_out) and torch.equal(attr.grad, r_ga) and torch.equal(barys.grad, r_gb)
        if with_delta:
            assert torch.equal(dl.grad, r_gb)                                # one gradient for barys and delta_barys


@pytest.mark.parametrize("req", list(itertools.product((False, True), repeat=3)))
def test_every_needs_input_grad_combination(req):
    from d3ga_amd.bary_interp import bary_interp
    P, K, C, V = 65, 4, 3, 5
    c = case(P, K, C, V)
    _, full_ga, full_gb = raw(c, P, K, C, V, True)
    attr, barys, dl = leaves(c, True, req)
    out = bary_interp(attr, c["binding"], barys, dl)
    assert out.requires_grad == any(req)
    if not any(req):
        return
    out.backward(c["dev"]["g_out"])
    for t, on, want in ((attr, req[0], full_ga), (barys, req[1], full_gb), (dl, req[2], full_gb)):
        assert (t.grad is None) == (not on)
        if on:
            assert torch.equal(t.grad, want)


@pytest.mark.parametrize("K", KS)
def test_non_contiguous_misaligned_and_float64_inputs(K):
    from d3ga_amd.bary_interp import bary_interp
    P, C, V = 257, 3, 300
    c = case(P, K, C, V)
    d = c["dev"]
    base = bary_interp(d["attr"], c["binding"], d["barys"], d["delta"])
    wide = torch.zeros(V, 2 * C, device=DEV)
    wide[:, ::2] = d["attr"]
    attr_nc = wide[:, ::2].requires_grad_(True)                              # stride 2 along the channels
    barys_nc = d["barys"].t().contiguous().t().requires_grad_(True)          # column-major
    flat = torch.zeros(P * K + 1, device=DEV)
    flat[1:] = d["delta"].reshape(-1)
    delta_off = flat[1:].view(P, K)                                          # contiguous, 4 bytes off a 16-byte boundary
    assert not attr_nc.is_contiguous() and not barys_nc.is_contiguous() and delta_off.data_ptr() % 16 == 4
    out = bary_interp(attr_nc, c["binding"], barys_nc, delta_off)
    assert torch.equal(out, base)
    out.backward(d["g_out"])
    _, r_ga, r_gb = raw(c, P, K, C, V, True)
    assert torch.equal(attr_nc.grad, r_ga) and torch.equal(barys_nc.grad, r_gb)
    # another float type is converted on the way in, its gradient on the way out
    attr64, barys64 = d["attr"].double().requires_grad_(True), d["barys"].double().requires_grad_(True)
    out64 = bary_interp(attr64, c["binding"], barys64, d["delta"])
    assert out64.dtype == torch.float32 and torch.equal(out64, base)
    out64.backward(d["g_out"])
    assert attr64.grad.dtype == torch.float64 and barys64.grad.dtype == torch.float64 and torch.equal(attr64.grad.float(), r_ga)
    # a non-contiguous upstream gradient
    attr, barys, dl = leaves(c)
    g_nc = d["g_out"].t().contiguous().t()
    bary_interp(attr, c["binding"], barys, dl).backward(g_nc)
    assert torch.equal(attr.grad, r_ga) and torch.equal(dl.grad, r_gb)


def test_one_dimensional_attr_returns_a_column():
    from d3ga_amd.bary_interp import bary_interp
    P, K, C, V = 1000, 4, 1, 5
    c = case(P, K, C, V)
    d = c["dev"]
    a1 = d["attr"][:, 0].clone().requires_grad_(True)
    out = bary_interp(a1, c["binding"], d["barys"], d["delta"])
    assert out.shape == (P, 1)
    out.backward(d["g_out"])
    r_out, r_ga, _ = raw(c, P, K, C, V, True)
    assert a1.grad.shape == (V,) and torch.equal(out, r_out) and torch.equal(a1.grad, r_ga[:, 0])


def test_shape_and_device_refusals():
    from d3ga_amd import D3GAError
    from d3ga_amd.bary_interp import BaryBinding, bary_interp
    c = case(65, 4, 3, 5)
    d, b = c["dev"], c["binding"]
    with pytest.raises(D3GAError):
        bary_interp(d["attr"][:4], b, d["barys"])                            # V of the binding
    with pytest.raises(D3GAError):
        bary_interp(torch.zeros(5, 9, device=DEV), b, d["barys"])            # C > 8
    with pytest.raises(D3GAError):
        bary_interp(d["attr"], b, d["barys"][:, :3])
    with pytest.raises(D3GAError):
        bary_interp(d["attr"], b, d["barys"], d["delta"][:-1])
    with pytest.raises(D3GAError):
        bary_interp(d["attr"], BaryBinding(c["cpu"]["rows"], n_rows=5), d["barys"])     # a plan built on the CPU
    with pytest.raises(D3GAError):
        bary_interp(d["attr"], d["rows"], d["barys"])                        # a table is not a binding


def test_graph_capture_of_forward_and_backward_replays_bit_identically():
    from d3ga_amd.bary_interp import bary_interp
    P, K, C, V = 1000, 3, 8, 300
    c = case(P, K, C, V)
    d = c["dev"]
    s_attr, s_barys, s_delta, s_up = (d[k].clone() for k in ("attr", "barys", "delta", "g_out"))

    def step(attr, barys, delta, up):
        attr, barys, delta = attr.detach().requires_grad_(True), barys.detach().requires_grad_(True), delta.detach().requires_grad_(True)
        out = bary_interp(attr, c["binding"], barys, delta)
        return (out.detach(),) + torch.autograd.grad(out, (attr, barys, delta), up)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step(s_attr, s_barys, s_delta, s_up)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                            # one linear chain of launches on one stream
        captured = step(s_attr, s_barys, s_delta, s_up)
    g = torch.Generator().manual_seed(9)
    new = [torch.randn(t.shape, generator=g).to(DEV) for t in (s_attr, s_barys, s_delta, s_up)]
    for static, n in zip((s_attr, s_barys, s_delta, s_up), new):
        static.copy_(n)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(captured, step(*new)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", ["shadow", "canonical", "mesh", "mesh_canonical"])
def test_reference_fixture_through_the_adapters(golden, name):
    """interp_cases.npz (the reference's own forwards) through cage_attr / mesh_means: within one bar of the float64
    restatement and within two of the reference's float32 results."""
    from d3ga_amd.bary_interp import cage_attr, mesh_means
    c = bary_ref.golden_cases(golden("interp_cases.npz"))[name]
    rows = bary_ref.final_rows(**c["bind"])
    K, C = rows.shape[1], 1 if c["attr"].dim() == 1 else c["attr"].shape[1]
    dev = lambda t: None if t is None else t.to(DEV)
    attr, barys, delta = dev(c["attr"]).requires_grad_(True), dev(c["barys"]), dev(c["delta"])
    if delta is not None:
        delta.requires_grad_(True)
    if "rows" in c["bind"]:
        out = mesh_means(attr, dev(c["bind"]["rows"]), barys, delta)
    else:
        out = cage_attr(attr, dev(c["bind"]["cells"]), dev(c["bind"]["cell_id"]), barys, delta, vertex_map=dev(c["bind"].get("vertex_map")))
    ref = bary_ref.interp_ref(c["attr"], rows, c["barys"], c["delta"], c["up"])
    bar = bary_ref.bars(ref, K, C)
    assert out.shape == c["out"].shape
    bary_ref.assert_within(f"{name} out vs float64", out, ref["out"], bar["out"])
    bary_ref.assert_within(f"{name} out vs reference", out, c["out"].double(), bar["out"], factor=2.0)
    if c["up"] is None:
        return
    out.backward(dev(c["up"]))
    assert attr.grad.shape == c["g_attr"].shape
    for what, got, key in (("g_attr", attr.grad, "g_attr"), ("g_barys", delta.grad, "g_barys")):
        bary_ref.assert_within(f"{name} {what} vs float64", got, ref[key], bar[key])
        bary_ref.assert_within(f"{name} {what} vs reference", got, c[key].double(), bar[key], factor=2.0)


def test_mesh_primitive_step_chains_the_rasterizer_gradient_into_the_mesh_points():
    """mesh_means -> render(scales, rotations) -> l1_loss -> backward on V = 30, P = 64, 64 x 64: the gradient at the mesh
    points (and at delta_bary) is, bit for bit, bary_interp's backward applied to the rasterizer's own means3D gradient -- the
    chain, not the rasterizer, is what this asserts."""
    from d3ga_amd import synthetic as syn
    from d3ga_amd.bary_interp import mesh_means
    from d3ga_amd.losses import l1_loss
    from d3ga_amd.renderer import render
    g = torch.Generator().manual_seed(11)
    V, F, P = 30, 40, 64
    faces = torch.stack([torch.randperm(V, generator=g)[:3] for _ in range(F)])
    face_ids = faces[torch.randint(0, F, (P,), generator=g)].to(DEV)
    points = (0.35 * torch.randn(V, 3, generator=g)).to(DEV).requires_grad_(True)
    barys = torch.rand(P, 3, generator=g)
    barys = (barys / barys.sum(1, keepdim=True)).to(DEV)
    delta = (0.05 * torch.tanh(torch.randn(P, 3, generator=g))).to(DEV).requires_grad_(True)
    means = mesh_means(points, face_ids, barys, delta)
    means.retain_grad()
    rot = torch.nn.functional.normalize(torch.randn(P, 4, generator=g), dim=1).to(DEV)
    pkg = {"means3D": means, "scales": torch.full((P, 3), 0.05, device=DEV), "rotations": rot, "cov3D_precomp": None,
           "opacities": torch.full((P, 1), 0.7, device=DEV), "shs": None, "rgb": torch.rand(P, 3, generator=g).to(DEV)}
    img = render(syn.make_batch(64, 64), pkg, torch.ones(3, device=DEV))["render"]
    assert img.shape == (3, 64, 64)
    l1_loss(img, torch.rand(3, 64, 64, generator=g).to(DEV)).backward()
    assert torch.isfinite(means.grad).all() and float(means.grad.abs().max()) > 0
    p2, d2 = points.detach().requires_grad_(True), delta.detach().requires_grad_(True)
    gp, gd = torch.autograd.grad(mesh_means(p2, face_ids, barys, d2), (p2, d2), means.grad)
    assert torch.equal(points.grad, gp) and torch.equal(delta.grad, gd)
    ref = bary_ref.interp_ref(points, face_ids, barys, delta, means.grad)
    bar = bary_ref.bars(ref, 3, 3)
    bary_ref.assert_within("mesh step g_points", points.grad, ref["g_attr"], bar["g_attr"])
    bary_ref.assert_within("mesh step g_delta", delta.grad, ref["g_barys"], bar["g_barys"])
