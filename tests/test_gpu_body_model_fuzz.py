"""Randomized and edge-case GPU parity of the SMPL / SMPL-X body model (d3ga_amd/body_model.py, csrc/body_model.hip)
against the float64 oracle (tests/smplx_ref.py), beyond the default settings of tests/test_gpu_body_model.py: random
kinematic trees of 2..64 joints (chains, stars, bushy and random shapes), 1..4000 vertices (ld tails of every length, 3V == ld),
1..8 skin weights per vertex with empty rows and vertex-less joints, every hand-PCA layout, B = 1..20 (every blend-kernel
instance and multi-launch), the rotation edges (exact zero, 1e-6, pi, 2 pi and beyond), optional inputs left out, broadcast
and narrow coefficient rows, and any subset of the outputs carrying a gradient.

Bars (those of test_gpu_body_model.py): forward |a - b| <= 1e-5 max|b| per output, A orthonormal, the constant bottom
rows of T and A exact; every gradient within the element-wise bar (tests/util.elementwise_excess <= 1); two backward calls
bitwise equal.  The bottom row of T is the ABI's constant (0, 0, 0, 1) (include/d3ga.h): the oracle's W A has
(0, 0, 0, sum_j w_vj) there, which differs only on vertices without weight, so the rows above it are what is compared.

D3GA_BODY_FUZZ_N seeds (default 6; the campaign form in tools/gpu_campaigns.sh runs 500)."""
import copy
import os

import numpy as np
import pytest
import torch

from d3ga_amd import synthetic as syn
from smplx_ref import RefSMPL, edge_rotations
from util import elementwise_excess

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("poses", "shapes", "expression", "Rh", "Th")
OUTS = ("verts", "T", "A", "bs")


# ---------------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------------
class Models:
    """Model files in one directory: the full-size SMPL-X model is generated and written once per module, and its layers
    (one per hand-PCA setting) and oracle are kept; every other model is written, loaded and dropped per case."""

    def __init__(self, root):
        self.root = root
        self.n = 0
        self._full = None
        self._full_layers = {}

    def _write(self, data, kind):
        self.n += 1
        d = os.path.join(self.root, f"m{self.n}")
        os.makedirs(d)
        path = os.path.join(d, ("SMPLX_NEUTRAL" if kind == "smplx" else "SMPL_NEUTRAL") + ".npz")
        syn.write_smpl_model(path, data)
        return path

    def layer(self, data, kind, pca=6, use_pca=True, flat=True):
        from d3ga_amd.body_model import SMPLlayer
        path = self._write(data, kind)
        try:
            layer = SMPLlayer(path, model_type=kind, num_pca_comps=pca, use_pca=use_pca, use_flat_mean=flat).to(DEV)
        finally:
            os.remove(path)
        return layer, RefSMPL(data, model_type=kind, num_pca_comps=pca if use_pca else 0, use_flat_mean=flat)

    def full_smplx(self, pca=6, use_pca=True, flat=True):
        from d3ga_amd.body_model import SMPLlayer
        if self._full is None:
            data = syn.smpl_model_data("smplx", seed=21)
            self._full = (data, self._write(data, "smplx"), RefSMPL(data, num_pca_comps=0))
        data, path, base = self._full
        key = (pca if use_pca else 0, flat)
        if key not in self._full_layers:
            self._full_layers[key] = SMPLlayer(path, model_type="smplx", num_pca_comps=pca, use_pca=use_pca,
                                               use_flat_mean=flat).to(DEV)
        ref = copy.copy(base)                 # the float64 arrays are shared; only the hand PCA differs
        n = key[0]
        ref.npca = n
        ref.hc = [torch.from_numpy(np.asarray(data["hands_components" + s], np.float64))[:n] for s in ("l", "r")]
        ref.hm = [torch.zeros(45, dtype=torch.float64) if flat else torch.from_numpy(np.asarray(data["hands_mean" + s],
                                                                                                  np.float64))
                  for s in ("l", "r")]
        ref.NUM_POSES = 75 + 2 * n if n > 0 else 3 * ref.J
        return self._full_layers[key], ref


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    return Models(str(tmp_path_factory.mktemp("smplx_fuzz")))


# ---------------------------------------------------------------------------------------------------------------------
# inputs and the comparison
# ---------------------------------------------------------------------------------------------------------------------
def draw_angles(rng, n, large=True):
    """(n, 3): per rotation an exact 0, 1e-6, 0.35-scale or (if `large`) 1.5 .. 6 rad, on a random axis."""
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    c = rng.choice(4, size=n, p=[0.2, 0.15, 0.45, 0.2] if large else [0.25, 0.2, 0.55, 0.0])
    mag = np.select([c == 0, c == 1, c == 2], [0.0, 1e-6, np.abs(0.35 * rng.normal(size=n))], rng.uniform(1.5, 6.0, size=n))
    return (d * mag[:, None]).astype(np.float32)


def make_inputs(layer, rng, B, full=True, large=True, expr="B", rh=True, th=True, shape_rows="B", shape_w=10, expr_w=10):
    """Float32 CPU inputs (poses, shapes, expression, Rh, Th); None where left out."""
    J = layer.J
    P = 3 * J if full else layer.NUM_POSES
    if full or layer.n_hand_pca == 0:
        poses = draw_angles(rng, B * J, large).reshape(B, 3 * J)
    else:                                 # compact: body / face joints as rotations, the hand PCA as coefficients
        nh = layer.n_hand_pca
        body = draw_angles(rng, B * 25, large).reshape(B, 75)
        pca = (rng.normal(size=(B, 2 * nh)) * (rng.random((B, 2 * nh)) > 0.2)).astype(np.float32)
        poses = np.concatenate([body[:, :66], pca, body[:, 66:]], axis=1)
    assert poses.shape == (B, P)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    nrow = lambda r: B if r == "B" else 1
    shapes = t(rng.normal(size=(nrow(shape_rows), shape_w)))
    e = None
    if layer.n_expr and expr is not None:
        e = t(rng.normal(size=(nrow(expr), expr_w)))
    Rh = t(draw_angles(rng, B, large)) if rh else None
    Th = t(rng.normal(size=(B, 3))) if th else None
    return t(poses), shapes, e, Rh, Th


def run(layer, ref, inp, which, seed):
    """Kernel and oracle forward, the loss sum_k <out_k, u_k> over the outputs in `which`, the kernel's gradients twice."""
    tk = [None if x is None else x.to(DEV).requires_grad_(True) for x in inp]
    tr = [None if x is None else x.double().requires_grad_(True) for x in inp]
    ok = layer(poses=tk[0], shapes=tk[1], Rh=tk[3], Th=tk[4], expression=tk[2])
    orr = ref(tr[0], tr[1], Rh=tr[3], Th=tr[4], expression=tr[2])
    g = torch.Generator().manual_seed(seed)
    ups = [torch.randn(o.shape, generator=g, dtype=torch.float64) for o in orr]
    lk = sum((ok[k] * ups[k].to(DEV).float()).sum() for k in which)
    lr = sum((orr[k] * ups[k]).sum() for k in which)
    req = [x for x in tk if x is not None]
    g1 = torch.autograd.grad(lk, req, retain_graph=True)
    g2 = torch.autograd.grad(lk, req)
    lr.backward()
    it1, it2 = iter(g1), iter(g2)
    gk = [None if x is None else next(it1) for x in tk]
    gk2 = [None if x is None else next(it2) for x in tk]
    return ok, orr, gk, gk2, [None if x is None else x.grad for x in tr]


def check(layer, ref, inp, which, seed, desc):
    ok, orr, gk, gk2, gr = run(layer, ref, inp, which, seed)
    for name, a, b in zip(OUTS, ok, orr):
        a, b = a.detach().double().cpu(), b.detach()
        if name == "T":
            assert torch.equal(a[..., 3, :], torch.tensor([0.0, 0, 0, 1], dtype=torch.float64).expand_as(a[..., 3, :])), \
                f"{desc}: T bottom row"
            a, b = a[..., :3, :], b[..., :3, :]
        err, top = float((a - b).abs().max()), float(b.abs().max())
        assert err <= 1e-5 * top, f"{desc}: {name} max error {err / max(top, 1e-300):.3e} of max|ref|"
    A = ok[2].detach().double().cpu()
    assert torch.equal(A[..., 3, :], torch.tensor([0.0, 0, 0, 1], dtype=torch.float64).expand_as(A[..., 3, :])), desc
    orth = float((A[..., :3, :3].transpose(-1, -2) @ A[..., :3, :3] - torch.eye(3, dtype=torch.float64)).abs().max())
    assert orth <= 64 * 2.0 ** -23, f"{desc}: A not orthonormal: {orth:.3e}"
    for name, a, a2, b, x in zip(NAMES, gk, gk2, gr, inp):
        if x is None:
            continue
        assert torch.equal(a, a2), f"{desc}: d{name} differs between two backward calls"
        a = a.detach().cpu()
        assert torch.isfinite(a).all(), f"{desc}: d{name} not finite"
        if b is None or float(b.abs().max()) == 0.0:        # None: the oracle's loss does not reach the input
            assert float(a.abs().max()) == 0.0, f"{desc}: d{name} should be zero"
            continue
        ex = elementwise_excess(a.numpy(), b.numpy())
        assert ex <= 1.0, f"{desc}: d{name} exceeds the element-wise bar x{ex:.2f}"


# ---------------------------------------------------------------------------------------------------------------------
# the fuzz
# ---------------------------------------------------------------------------------------------------------------------
# vertex counts at the edges of the ld = ceil(3V / 2048) * 2048 layout: V = 1 (nvb = 1, the row is nearly all tail), 3V one
# short of / one past 2048, 3V == 4096 +- 2, 3V == 6144 == ld exactly (the tail-zeroing loop runs zero times)
EDGE_V = (1, 2, 682, 683, 1365, 1366, 2048)


def draw(seed):
    rng = np.random.default_rng(7000 + seed)
    c = {"seed": seed, "full_size": seed % 5 == 0}
    c["kind"] = "smplx" if c["full_size"] or rng.random() < 0.5 else "smpl"
    if c["full_size"]:
        c["J"], c["tree"], c["V"], c["S"] = 55, "random (the module's full-size model)", 10475, 400
    elif c["kind"] == "smpl":
        c["J"] = int(rng.integers(2, 65))
        c["tree"] = str(rng.choice(["random", "chain", "bushy", "star"]))
    else:
        c["J"], c["tree"] = 55, str(rng.choice(["random", "chain", "bushy"]))
    if not c["full_size"]:
        c["V"] =int(rng.choice(EDGE_V)) if rng.random() < 0.3 else int(rng.integers(1, 4001))
        c["S"] = (int(rng.choice([20, 400])) if c["kind"] == "smplx" else 10)
        c["max_weights"] = int(rng.integers(1, 9))
        c["empty_rows"] = float(rng.choice([0.0, 0.1]))
        c["empty_joints"] = float(rng.choice([0.0, 0.2]))
        c["model_seed"] = int(rng.integers(0, 2 ** 31))
    if c["kind"] == "smplx":
        c["pca"] = int(rng.choice([1, 6, 12, 44, 45]))
        c["use_pca"] = bool(rng.random() < 0.8)
        c["flat"] = bool(rng.random() < 0.5)
    c["B"] = int(rng.integers(1, 21))
    c["full"] = bool(rng.random() < 0.5)
    c["large"] = bool(rng.random() < 0.5)
    c["shape_rows"] = str(rng.choice(["B", "1"]))
    c["shape_w"] = int(rng.choice([10, int(rng.integers(1, 10))]))
    c["expr"] = None if rng.random() < 0.3 else str(rng.choice(["B", "1"]))
    c["expr_w"] = int(rng.choice([10, int(rng.integers(1, 10))]))
    c["rh"], c["th"] = bool(rng.random() < 0.7), bool(rng.random() < 0.7)
    which = [k for k in range(4) if rng.random() < 0.5]
    c["which"] = tuple(which) if which else (int(rng.integers(0, 4)),)
    return c, rng


def build(models, c):
    pca = dict(pca=c.get("pca", 6), use_pca=c.get("use_pca", True), flat=c.get("flat", True))
    if c["full_size"]:
        return models.full_smplx(**pca)
    data = syn.smpl_model_data(c["kind"], seed=c["model_seed"], V=c["V"], J=c["J"], tree=c["tree"], max_depth=c["J"],
                               n_shapedirs=c["S"] if c["kind"] == "smplx" else None, max_weights=c["max_weights"],
                               empty_rows=c["empty_rows"], empty_joints=c["empty_joints"])
    return models.layer(data, c["kind"], **pca)


@pytest.mark.parametrize("seed", range(int(os.environ.get("D3GA_BODY_FUZZ_N", "6"))))
def test_body_model_fuzz(models, seed):
    c, rng = draw(seed)
    layer, ref = build(models, c)
    desc = "draw " + ", ".join(f"{k}={v}" for k, v in c.items())
    inp = make_inputs(layer, rng, c["B"], full=c["full"], large=c["large"], expr=c["expr"], rh=c["rh"], th=c["th"],
                      shape_rows=c["shape_rows"], shape_w=c["shape_w"], expr_w=c["expr_w"])
    check(layer, ref, inp, c["which"], seed, desc)


# ---------------------------------------------------------------------------------------------------------------------
# fixed cases: the edges every default run covers
# ---------------------------------------------------------------------------------------------------------------------
_fixed = {}


def fixed_model(models, name):
    """Small models of the fixed cases (built once per module)."""
    if name not in _fixed:
        kw = {"smplx": dict(kind="smplx", seed=31, V=1500, n_shapedirs=20),
              "chain64": dict(kind="smpl", seed=32, V=900, J=64, tree="chain"),
              "star64": dict(kind="smpl", seed=33, V=900, J=64, tree="star"),
              "v1": dict(kind="smplx", seed=34, V=1, n_shapedirs=20),
              "v1_unweighted": dict(kind="smpl", seed=37, V=1, empty_rows=1.0),
              "v_ld": dict(kind="smpl", seed=35, V=2048),
              "sparse": dict(kind="smpl", seed=36, V=700, J=40, tree="bushy", max_weights=8, empty_rows=0.15,
                             empty_joints=0.25)}[name]
        kind = kw.pop("kind")
        _fixed[name] = (syn.smpl_model_data(kind, **kw), kind)
    data, kind = _fixed[name]
    return data, kind


def fixed_layer(models, name, **pca):
    key = (name, tuple(sorted(pca.items())))
    if key not in _fixed:
        data, kind = fixed_model(models, name)
        _fixed[key] = models.layer(data, kind, **pca)
    return _fixed[key]


@pytest.mark.parametrize("B", [4, 5, 6, 7, 8, 9, 16, 17])
def test_backward_every_blend_instance(models, B):
    """blend_bwd_kernel<NB> for NB = 4..8 and the launches after the first (frames 8.., 16..): the gradients of all outputs."""
    layer, ref = fixed_layer(models, "smplx")
    rng = np.random.default_rng(100 + B)
    check(layer, ref, make_inputs(layer, rng, B, full=False), (0, 1, 2, 3), B, f"B={B}")


PCA_CASES = [(n, flat, full) for n in (1, 6, 12) for flat in (True, False) for full in (False, True)] + \
            [(45, flat, True) for flat in (True, False)]


@pytest.mark.parametrize("n,flat,full", PCA_CASES)
def test_hand_pca_layouts(models, n, flat, full):
    """num_pca_comps x {flat mean, hands_mean} x {compact, full pose}.  With 45 components the compact width 75 + 90 is
    3J: such a pose is the full layout (the documented `(B,3J)` form), not PCA coefficients."""
    layer, ref = fixed_layer(models, "smplx", pca=n, flat=flat)
    assert layer.n_hand_pca == n and layer.NUM_POSES == 75 + 2 * n
    rng = np.random.default_rng(200 + n)
    inp = make_inputs(layer, rng, 3, full=full)
    check(layer, ref, inp, (0, 1, 2, 3), n, f"num_pca_comps={n}, use_flat_mean={flat}, full={full}")


def test_hand_pca_off(models):
    layer, ref = fixed_layer(models, "smplx", use_pca=False)
    assert layer.n_hand_pca == 0 and layer.NUM_POSES == 165
    check(layer, ref, make_inputs(layer, np.random.default_rng(210), 3), (0, 1, 2, 3), 210, "use_pca=False")


@pytest.mark.parametrize("missing", ["Rh", "Th", "expression", "all"])
def test_optional_inputs_left_out(models, missing):
    """Rh / Th / expression = None (the kernels' NULL branches) with gradients into the rest."""
    layer, ref = fixed_layer(models, "smplx")
    gone = {"Rh", "Th", "expression"} if missing == "all" else {missing}
    inp = make_inputs(layer, np.random.default_rng(300), 3, expr=None if "expression" in gone else "B",
                      rh="Rh" not in gone, th="Th" not in gone)
    for which in ((0,), (0, 1, 2, 3)):
        check(layer, ref, inp, which, 301, f"{missing}=None, upstream {which}")


@pytest.mark.parametrize("full", [False, True])
def test_rotation_edges(models, full):
    """Every joint and Rh from the angle edge set (exact zero beside nonzero angles in one frame, 1e-7 .. 1e-3, pi, 2 pi and
    past it) at J = 55."""
    layer, ref = fixed_layer(models, "smplx")
    rng = np.random.default_rng(400)
    B = 4
    r = edge_rotations(rng, B * 56)
    inp = list(make_inputs(layer, rng, B, full=True))
    inp[0] = torch.from_numpy(r[:B * 55].reshape(B, 165))
    inp[3] = torch.from_numpy(r[B * 55:B * 56])
    if not full:                          # the compact layout: the same body / face rotations, PCA coefficients for the hands
        p = inp[0]
        pca = torch.from_numpy(rng.normal(size=(B, 12)).astype(np.float32))
        inp[0] = torch.cat([p[:, :66], pca, p[:, 66:75]], dim=1)
    check(layer, ref, tuple(inp), (0, 1, 2, 3), 401, f"angle edge set, full={full}")


@pytest.mark.parametrize("name", ["chain64", "star64"])
def test_64_joint_trees(models, name):
    """J = D3GA_BODY_MAX_JOINTS as a 64-deep chain (64 levels) and as a star (63 children of the root, one level)."""
    layer, ref = fixed_layer(models, name)
    assert layer.J == 64 and layer.n_levels == (64 if name == "chain64" else 2)
    check(layer, ref, make_inputs(layer, np.random.default_rng(500), 3, large=False), (0, 1, 2, 3), 501, name)


@pytest.mark.parametrize("name", ["v1", "v1_unweighted", "v_ld", "sparse"])
def test_vertex_layout_edges(models, name):
    """V = 1 (the dirs rows are nearly all zero tail, one skin workgroup), V = 1 without any skin weight (empty CSR arrays:
    campaign seeds 201, 352 and 383 found the layer handing NULL pointers to the ABI), 3V == ld (no tail to zero), and a
    model with up to 8 weights per vertex, vertices without weight and joints without vertices."""
    layer, ref = fixed_layer(models, name)
    if name == "v1_unweighted":
        assert float(layer.weights.abs().max()) == 0.0
    if name == "v_ld":
        assert 3 * layer.V == layer.ld
    if name == "sparse":
        W = layer.weights.cpu()
        assert (W.sum(1) == 0).any() and (W.sum(0) == 0).any() and int((W > 0).sum(1).max()) > 4
    for B in (1, 9):
        check(layer, ref, make_inputs(layer, np.random.default_rng(600 + B), B), (0, 1, 2, 3), 601, f"{name}, B={B}")


def test_graph_replay_and_determinism_b11(models):
    """B = 11 (two launches of each blend kernel) captured in one graph with the backward, replayed with new inputs: equal
    bit for bit to the eager call, which is itself repeatable and matches the oracle."""
    layer, ref = fixed_layer(models, "smplx")
    B = 11
    rng = np.random.default_rng(700)
    inp = make_inputs(layer, rng, B, full=False)
    new = make_inputs(layer, rng, B, full=False)
    check(layer, ref, new, (0, 1, 2, 3), 701, "B=11 eager")
    poses, shapes, expr, Rh, Th = [x.to(DEV) for x in inp]
    g = torch.Generator().manual_seed(3)
    ups = [torch.randn(s, generator=g).to(DEV) for s in ((B, layer.V, 3), (B, layer.V, 4, 4), (B, layer.J, 4, 4),
                                                          (B, layer.V, 3))]

    def step(p, s, e, r, t):
        p, s, r, t = (x.requires_grad_(True) for x in (p, s, r, t))
        out = layer(poses=p, shapes=s, Rh=r, Th=t, expression=e)
        grads = torch.autograd.grad(sum((o * u).sum() for o, u in zip(out, ups)), (p, s, r, t))
        return [o.detach() for o in out] + list(grads)

    sp, ss, sr, st = poses.clone(), shapes.clone(), Rh.clone(), Th.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step(sp.detach(), ss.detach(), expr, sr.detach(), st.detach())
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step(sp.detach(), ss.detach(), expr, sr.detach(), st.detach())
    for dst, src in zip((sp, ss, sr, st), (new[0], new[1], new[3], new[4])):
        dst.copy_(src.to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    eager = [step(new[0].to(DEV), new[1].to(DEV), expr, new[3].to(DEV), new[4].to(DEV)) for _ in range(2)]
    for k, (a, b, c) in enumerate(zip(captured, *eager)):
        assert torch.equal(b, c), f"eager output {k} not repeatable"
        assert torch.equal(a, b), f"graph replay output {k} differs from the eager call"
