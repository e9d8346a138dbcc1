"""GPU parity of the SMPL / SMPL-X body model (d3ga_amd/body_model.py, csrc/body_model.hip) against the float64 oracle
(tests/smplx_ref.py) on synthetic model files of SMPL-X and SMPL size: forward outputs, gradients from every output into
poses, shapes, expression, Rh and Th, determinism, the pure global transform, graph capture and the reference's call
sequence through `compat`.  Forward bar |a - b| <= 1e-5 max|b|; gradient bar element-wise (tests/util.elementwise_excess)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from d3ga_amd import synthetic as syn
from smplx_ref import RefSMPL
from util import elementwise_excess

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("smplx_gpu")
    out = {}
    for name, kind, kw in (("smplx", "smplx", {}), ("smpl", "smpl", {}), ("chain", "smplx", {"chain": True})):
        data = syn.smpl_model_data(kind, seed={"smplx": 11, "smpl": 12, "chain": 13}[name], **kw)
        sub = d / name
        sub.mkdir()
        fname = ("SMPLX_NEUTRAL" if kind == "smplx" else "SMPL_NEUTRAL") + (".npz" if name == "smpl" else ".pkl")
        syn.write_smpl_model(str(sub / fname), data, sparse_regressor=(name == "chain"))
        out[name] = (data, str(sub), kind)
    return out


_layers = {}


def layer_of(models, name):
    if name not in _layers:
        from d3ga_amd.body_model import SMPLlayer
        data, path, kind = models[name]
        _layers[name] = (SMPLlayer(path, model_type=kind, gender="neutral", use_joints=True, regressor_path=None).to(DEV),
                         RefSMPL(data, model_type=kind))
    return _layers[name]


def make_inputs(layer, B, full=False, seed=0, star=False, rh=True):
    g = torch.Generator().manual_seed(seed)
    P = 3 * layer.J if full else layer.NUM_POSES
    if star:
        poses = torch.zeros(B, P)
        poses[:, 5], poses[:, 8] = math.pi / 6, -math.pi / 6
    else:
        poses = 0.35 * torch.randn(B, P, generator=g)
    shapes = torch.randn(B, 10, generator=g)
    expr = torch.randn(B, 10, generator=g) if layer.n_expr else None
    Rh = (0.8 * torch.randn(B, 3, generator=g)) if rh else torch.zeros(B, 3)
    Th = torch.randn(B, 3, generator=g)
    return poses, shapes, expr, Rh, Th


def run_kernel(layer, inp, grad=False):
    t = [None if x is None else x.to(DEV).requires_grad_(grad) for x in inp]
    out = layer(poses=t[0], shapes=t[1], Rh=t[3], Th=t[4], expression=t[2])
    return t, out


def run_ref(ref, inp, grad=False):
    t = [None if x is None else x.double().requires_grad_(grad) for x in inp]
    out = ref(t[0], t[1], Rh=t[3], Th=t[4], expression=t[2])
    return t, out


def fwd_close(a, b, bar=1e-5):
    a, b = a.detach().double().cpu(), b.detach().double()
    err = float((a - b).abs().max())
    return err <= bar * float(b.abs().max()), err / float(b.abs().max())


def assert_forward(layer, ref, inp):
    _, got = run_kernel(layer, inp)
    _, want = run_ref(ref, inp)
    for name, a, b in zip(("verts", "T", "A", "bs"), got, want):
        ok, rel = fwd_close(a, b)
        assert ok, f"{name}: max error {rel:.3e} of max|ref|"
    R = got[2][..., :3, :3].double()
    eye = torch.eye(3, dtype=torch.float64, device=R.device)
    orth = float((R.transpose(-1, -2) @ R - eye).abs().max())
    assert orth <= 64 * 2.0 ** -23, f"A not orthonormal: {orth:.3e}"
    assert torch.equal(got[2][..., 3, :].cpu(), torch.tensor([0.0, 0, 0, 1]).expand_as(got[2][..., 3, :].cpu()))
    return got


@pytest.mark.parametrize("B,full", [(1, False), (3, False), (1, True), (3, True)])
def test_forward_parity_smplx(models, B, full):
    layer, ref = layer_of(models, "smplx")
    assert_forward(layer, ref, make_inputs(layer, B, full=full, seed=B + 10 * full))


def test_forward_parity_smpl(models):
    layer, ref = layer_of(models, "smpl")
    assert layer.NUM_POSES == 72
    assert_forward(layer, ref, make_inputs(layer, 2, seed=3))


def test_forward_parity_deep_chain(models):
    layer, ref = layer_of(models, "chain")
    assert layer.n_levels == 55
    assert_forward(layer, ref, make_inputs(layer, 2, seed=4))


def test_forward_batch_beyond_one_launch(models):
    """B = 11: the blend passes take 8 frames per launch."""
    layer, ref = layer_of(models, "smplx")
    assert_forward(layer, ref, make_inputs(layer, 11, seed=5))


def _grads(layer, ref, inp, which, seed):
    tk, ok = run_kernel(layer, inp, grad=True)
    tr, orr = run_ref(ref, inp, grad=True)
    g = torch.Generator().manual_seed(seed)
    ups = [torch.randn(o.shape, generator=g, dtype=torch.float64) for o in orr]
    lk = sum((o * u.to(DEV).float()).sum() for k, (o, u) in enumerate(zip(ok, ups)) if k in which)
    lr = sum((o * u).sum() for k, (o, u) in enumerate(zip(orr, ups)) if k in which)
    lk.backward()
    lr.backward()
    return [(None if a is None else a.grad, None if b is None else b.grad) for a, b in zip(tk, tr)]


GRAD_CASES = {"verts": (0,), "T": (1,), "A": (2,), "bs": (3,), "all": (0, 1, 2, 3)}


@pytest.mark.parametrize("case", list(GRAD_CASES))
@pytest.mark.parametrize("B,full,star", [(1, False, False), (3, True, False), (2, False, True)])
def test_gradients_match_oracle(models, case, B, full, star):
    layer, ref = layer_of(models, "smplx")
    inp = make_inputs(layer, B, full=full, seed=20 + B, star=star)
    names = ("poses", "shapes", "expression", "Rh", "Th")
    for name, (a, b) in zip(names, _grads(layer, ref, inp, GRAD_CASES[case], seed=7)):
        if b is None:
            assert a is None or float(a.abs().max()) == 0.0, name
            continue
        assert a is not None, name
        a = a.detach().cpu()
        assert torch.isfinite(a).all(), name
        if float(b.abs().max()) == 0.0:
            assert float(a.abs().max()) == 0.0, name
            continue
        ex = elementwise_excess(a.numpy(), b.numpy())
        assert ex <= 1.0, f"d{name} ({case}) exceeds the element-wise bar x{ex:.2f}"


@pytest.mark.parametrize("name", ["smpl", "chain"])
def test_gradients_match_oracle_other_models(models, name):
    layer, ref = layer_of(models, name)
    inp = make_inputs(layer, 2, seed=30)
    for nm, (a, b) in zip(("poses", "shapes", "expression", "Rh", "Th"), _grads(layer, ref, inp, (0, 1, 2, 3), seed=8)):
        if b is None:
            continue
        ex = elementwise_excess(a.detach().cpu().numpy(), b.numpy())
        assert ex <= 1.0, f"{name}: d{nm} exceeds the element-wise bar x{ex:.2f}"


def test_broadcast_shapes_gradient_sums_over_batch(models):
    layer, ref = layer_of(models, "smplx")
    poses, shapes, expr, Rh, Th = make_inputs(layer, 3, seed=40)
    inp = (poses, shapes[:1], expr[:1], Rh, Th)
    for nm, (a, b) in zip(("poses", "shapes", "expression", "Rh", "Th"), _grads(layer, ref, inp, (0, 1, 2, 3), seed=9)):
        assert a.shape == b.shape, nm
        ex = elementwise_excess(a.detach().cpu().numpy(), b.numpy())
        assert ex <= 1.0, f"d{nm} exceeds the element-wise bar x{ex:.2f}"


def test_backward_is_deterministic(models):
    layer, _ = layer_of(models, "smplx")
    inp = make_inputs(layer, 3, seed=50)
    res = []
    for _ in range(2):
        t, out = run_kernel(layer, inp, grad=True)
        g = torch.Generator().manual_seed(1)
        loss = sum((o * torch.randn(o.shape, generator=g).to(DEV)).sum() for o in out)
        loss.backward()
        res.append([x.grad.clone() for x in t])
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_pure_global_transform(models):
    layer, _ = layer_of(models, "smplx")
    poses, shapes, expr, Rh, Th = make_inputs(layer, 2, seed=60)
    _, (v0, T0, A0, bs0) = run_kernel(layer, (poses, shapes, expr, torch.zeros(2, 3), torch.zeros(2, 3)))
    _, (v1, T1, A1, bs1) = run_kernel(layer, (poses, shapes, expr, Rh, Th))
    assert torch.equal(T0, T1) and torch.equal(A0, A1) and torch.equal(bs0, bs1)
    from d3ga_amd.cage_deform import batch_rodrigues
    R = batch_rodrigues(Rh.double())
    want = v0.double().cpu() @ R.transpose(1, 2) + Th.double()[:, None]
    err = float((v1.double().cpu() - want).abs().max())
    assert err <= 8 * 2.0 ** -23 * float(want.abs().max()), err


def test_graph_capture_replays_with_new_inputs(models):
    layer, _ = layer_of(models, "smplx")
    inp = make_inputs(layer, 2, seed=70)
    poses, shapes, expr, Rh, Th = [x.to(DEV) for x in inp]
    g = torch.Generator().manual_seed(2)
    ups = [torch.randn(s, generator=g).to(DEV) for s in ((2, layer.V, 3), (2, layer.V, 4, 4), (2, layer.J, 4, 4), (2, layer.V, 3))]

    def step(p, s, e, r, t):
        p, r, t = p.requires_grad_(True), r.requires_grad_(True), t.requires_grad_(True)
        out = layer(poses=p, shapes=s, Rh=r, Th=t, expression=e)
        gp, gr, gt = torch.autograd.grad(sum((o * u).sum() for o, u in zip(out, ups)), (p, r, t))
        return [o.detach() for o in out] + [gp, gr, gt]

    sp, sr, st = poses.clone(), Rh.clone(), Th.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step(sp.detach(), shapes, expr, sr.detach(), st.detach())
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step(sp.detach(), shapes, expr, sr.detach(), st.detach())
    new = make_inputs(layer, 2, seed=71)
    sp.copy_(new[0].to(DEV))
    sr.copy_(new[3].to(DEV))
    st.copy_(new[4].to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    eager = step(new[0].to(DEV), shapes, expr, new[3].to(DEV), new[4].to(DEV))
    for a, b in zip(captured, eager):
        assert torch.equal(a, b)


def test_reference_call_sequence_through_compat(models):
    """lib/smplman.py:68-74 builds the layer, Smplman.get (:172-180) calls it with keywords and Rh zeroed, Smplman.deform
    (:155-171) skins the cage with A and bs[:, nn_ids]: here through d3ga_amd.cage_deform.lbs_cage with K-sparse weights."""
    data, path, _ = models["smplx"]
    compat = os.path.join(ROOT, "compat")
    sys.path.insert(0, compat)
    try:
        for k in [m for m in sys.modules if m.split(".")[0] == "tetra_sampler"]:
            del sys.modules[k]
        from tetra_sampler.body_model import SMPLlayer
    finally:
        sys.path.remove(compat)
    layer = SMPLlayer(path, model_type="smplx", gender="neutral", use_joints=True, regressor_path=None).cuda()
    ref = RefSMPL(data)
    poses, shapes, expr, Rh, Th = make_inputs(layer, 1, seed=80)
    batch = {"poses": poses.to(DEV), "shapes": shapes.to(DEV), "expression": expr.to(DEV), "Rh": Rh.to(DEV), "Th": Th.to(DEV)}
    _, T, A, bs = layer(poses=batch["poses"], shapes=batch["shapes"], Rh=batch["Rh"] * 0, Th=batch["Th"] * 0,
                        expression=batch["expression"])
    _, Tr, Ar, bsr = ref(poses.double(), shapes.double(), Rh=torch.zeros(1, 3, dtype=torch.float64),
                         Th=torch.zeros(1, 3, dtype=torch.float64), expression=expr.double())
    # the cage: a subset of template vertices, K-sparse weights from the CSR rows
    rng = np.random.default_rng(0)
    nn = torch.from_numpy(np.sort(rng.choice(layer.V, size=3000, replace=False)))
    W = layer.weights.cpu()[nn]
    K = int((W > 0).sum(1).max())
    sw, si = torch.topk(W, K, dim=1)
    si = si.to(torch.int32)
    tmpl = layer.v_template.cpu()[nn] + 0.01 * torch.from_numpy(rng.normal(size=(len(nn), 3))).float()
    from d3ga_amd.cage_deform import lbs_cage, batch_rodrigues
    from oracle import deform as od
    Rm, Tv = batch_rodrigues(Rh.to(DEV)), Th.to(DEV)
    got = lbs_cage(tmpl.to(DEV), bs[0, nn.to(DEV)], A[0], si.to(DEV), sw.to(DEV), Rm[0], Tv[0])
    want = od.lbs_cage(tmpl.double(), bsr[0, nn], Ar[0], si.long(), sw.double(), batch_rodrigues(Rh.double())[0], Th.double()[0])
    ok, rel = fwd_close(got, want)
    assert ok, rel
