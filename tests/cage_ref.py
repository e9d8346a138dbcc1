"""Float64 side of tests/test_gpu_cage_paths.py: random cage bindings, the oracle chain lbs_cage -> cage_deform (oracle.deform)
with every gradient, the element-wise bars of test_cage_deform_fuzz, and output buffers with guard bands (float32: GuardedBuffer;
uint32 words: GuardedWords, also used by tests/test_gpu_mlp_paths.py).  CPU only, no GPU call in here except the guarded
buffers' allocation and checks."""
import numpy as np
import torch

from oracle import deform as od

GUARD = 64                      # floats on either side of a guarded output
FILL = 0x7FC0DEAD               # a quiet NaN with a payload no kernel produces


def make_case(seed, V, T, P, K=4, J=7, *, vertices_in_tets=None, sort_ids=True, one_tet=False):
    """Random binding and inputs (float32 / int32 CPU tensors), one dict.  Tetrahedra take their corners from the first
    `vertices_in_tets` vertices (default all); the canonical gradient is drawn directly as I + 0.3 randn per TETRAHEDRON
    (`cg_tet`; `cg` = its per-Gaussian copy), so no case depends on a random tetrahedron being invertible.  `scales_log` and
    `scales` are two independent inputs (log-scales for scale_activation="exp", activated scales without)."""
    g = torch.Generator().manual_seed(seed)
    nv = V if vertices_in_tets is None else vertices_in_tets
    tetras = torch.stack([torch.randperm(nv, generator=g)[:4] for _ in range(T)]).to(torch.int32) if T else torch.zeros(0, 4, dtype=torch.int32)
    tid = torch.zeros(P, dtype=torch.int64) if one_tet else torch.randint(0, max(T, 1), (P,), generator=g)
    if sort_ids:
        tid = torch.sort(tid)[0]
    tid = tid.to(torch.int32)
    idx = torch.randint(0, J, (V, K), generator=g).to(torch.int32)
    w = torch.rand(V, K, generator=g)
    w = w / w.sum(1, keepdim=True) if V else w
    cg_tet = torch.eye(3) + 0.3 * torch.randn(T, 3, 3, generator=g)
    barys = torch.rand(P, 4, generator=g)
    c = dict(V=V, T=T, P=P, K=K, J=J, tetras=tetras, tid=tid, idx=idx, w=w,
             tmpl=torch.randn(V, 3, generator=g), delta=0.05 * torch.randn(V, 3, generator=g),
             A=torch.eye(4).repeat(J, 1, 1) + 0.3 * torch.randn(J, 4, 4, generator=g),
             Rh=torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))[0].float(), Th=torch.randn(3, generator=g),
             tp=torch.randn(V, 3, generator=g), cg_tet=cg_tet, cg=cg_tet[tid.long()].contiguous(),
             barys=barys / barys.sum(1, keepdim=True) if P else barys, dbary=0.05 * torch.randn(P, 4, generator=g),
             scales_log=0.3 * torch.randn(P, 3, generator=g) - 2.0, scales=0.05 + 0.2 * torch.rand(P, 3, generator=g),
             rots=torch.randn(P, 4, generator=g),
             gm=torch.randn(P, 3, generator=g), gc=torch.randn(P, 6, generator=g), gt=torch.randn(V, 3, generator=g))
    c["A"][:, 3] = torch.tensor([0.0, 0.0, 0.0, 1.0])
    return c


def touched_vertices(c):
    """bool (V): the vertices some Gaussian's tetrahedron has as a corner."""
    t = torch.zeros(c["V"], dtype=torch.bool)
    if c["P"]:
        t[c["tetras"].long()[c["tid"].long()].reshape(-1)] = True
    return t


def _one(c, *, exp, dbary, rh, th, skin, use, eps, draw):
    ge = torch.Generator().manual_seed(4242 + 1000 * draw)

    def leaf(t):
        t = t.double()
        if eps:
            t = t * (1.0 + eps * (2.0 * torch.rand(t.shape, generator=ge).double() - 1.0))
        return t.requires_grad_(True)
    idx, w = c["idx"].long(), leaf(c["w"]).detach()
    tmpl, delta, A = leaf(c["tmpl"]), leaf(c["delta"]), leaf(c["A"])
    Rh, Th = (leaf(c["Rh"]) if rh else None), (leaf(c["Th"]) if th else None)
    out = od.lbs_cage(tmpl, delta, A, idx, w, Rh, Th) if (skin and c["V"]) else None
    tp = out.detach().clone().requires_grad_(True) if skin == "chain" and out is not None else leaf(c["tp"])
    b, d, r = leaf(c["barys"]), leaf(c["dbary"]), leaf(c["rots"])
    s = leaf(c["scales_log"] if exp else c["scales"])
    cg = leaf(c["cg"]).detach()
    m, cv = od.cage_deform(tp, c["tetras"].long(), c["tid"].long(), (b + d) if dbary else b, cg, torch.exp(s) if exp else s, r)
    loss = tp.sum() * 0.0
    if "m" in use:
        loss = loss + (m * c["gm"].double()).sum()
    if "c" in use:
        loss = loss + (cv * c["gc"].double()).sum()
    if "t" in use:
        loss = loss + (tp * c["gt"].double()).sum()
    loss.backward()
    z = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    res = dict(m=m.detach(), c=cv.detach(), tp=tp.detach(), g_tp=z(tp), g_barys=z(b), g_scales=z(s), g_rots=z(r))
    if out is not None:
        out.backward(res["g_tp"])
        res.update(g_delta=z(delta), g_tmpl=z(tmpl), A=z(A), Rh=None if Rh is None else z(Rh), Th=None if Th is None else z(Th))
    return res


def reference(c, *, exp=False, dbary=False, rh=False, th=False, skin=None, use="mc"):
    """The float64 oracle on the float32 inputs of case `c`, and per entry the largest movement of four evaluations with every
    float input moved by one relative float32 rounding (6e-8) -> (values, moved).
    skin: None = cage_deform on c["tp"]; "tail" = the same, and its vertex gradient carried through the skinning backward
    (what d3ga_cage_deform_bwd's skin / pose descriptors compute); "chain" = tetpoints are lbs_cage's output (lbs_cage_deform).
    use: which of sum(means gm), sum(cov6 gc), sum(tetpoints gt) the loss has.  Entries: m, c, tp, g_tp, g_barys (= the
    delta_barys gradient), g_scales, g_rots, and with skin g_delta, g_tmpl, A, Rh, Th (the pose gradients, keyed as check_pose)."""
    kw = dict(exp=exp, dbary=dbary, rh=rh, th=th, skin=skin, use=use)
    val = _one(c, eps=0.0, draw=0, **kw)
    moved = {k: torch.zeros_like(v) for k, v in val.items() if v is not None}
    for d in range(4):
        alt = _one(c, eps=6e-8, draw=d, **kw)
        for k in moved:
            moved[k] = torch.maximum(moved[k], (alt[k] - val[k]).abs())
    return val, moved


def excess(got, ref, key, floor=1e-6, extra_rel=0.0):
    """The bar of test_cage_deform_fuzz: worst |got - ref| / (1e-3 |ref| + floor max|ref| + 4 moved); <= 1 passes.  floor = 1e-5
    for the vertex-summed gradients.  extra_rel: a measured float32 summation spread, relative to max|ref| (item A only)."""
    val, moved = ref
    b = val[key].numpy()
    a = got.detach().cpu().double().numpy().reshape(b.shape)
    if b.size == 0:
        return 0.0
    allow = 1e-3 * np.abs(b) + max(floor, extra_rel) * np.abs(b).max() + 4.0 * moved[key].numpy() + 1e-300
    assert np.isfinite(a).all(), f"{key}: non-finite values"
    return float((np.abs(a - b) / allow).max())


def vertex_terms(c, *, exp, dbary):
    """The float64 (Gaussian, corner) terms of the vertex gradient, (4P,3), and their vertices (4P): what the product sums."""
    corners = c["tp"].double()[c["tetras"].long()][c["tid"].long()].requires_grad_(True)          # (P,4,3)
    b = c["barys"].double() + (c["dbary"].double() if dbary else 0.0)
    s = torch.exp(c["scales_log"].double()) if exp else c["scales"].double()
    J = od.tet_edge_matrix(corners) @ c["cg"].double()
    cov = J @ od.covariance_from_scale_rot(s, c["rots"].double()) @ J.transpose(1, 2)
    m = (corners * b[:, :, None]).sum(1)
    ((m * c["gm"].double()).sum() + (od.pack_sym6(cov) * c["gc"].double()).sum()).backward()
    return corners.grad.reshape(-1, 3), c["tetras"].long()[c["tid"].long()].reshape(-1)


def float32_order_spread(c, *, exp, dbary):
    """max |sum in item order - sum in reverse item order| over the vertex gradient, both accumulated in float32 from the float64
    terms rounded to float32, relative to the largest float64 element: what two float32 implementations that only differ in the
    order of a vertex's sum can disagree by."""
    terms, vid = vertex_terms(c, exp=exp, dbary=dbary)
    t32, v = terms.float().numpy(), vid.numpy()
    fwd, rev = np.zeros((c["V"], 3), np.float32), np.zeros((c["V"], 3), np.float32)
    np.add.at(fwd, v, t32)
    np.add.at(rev, v[::-1], t32[::-1])
    exact = np.zeros((c["V"], 3))
    np.add.at(exact, v, terms.numpy())
    return float(np.abs(fwd.astype(np.float64) - rev).max() / np.abs(exact).max())


class GuardedBuffer:
    """An output (shape, float32) in the middle of a larger device buffer filled with a NaN bit pattern: `t` is the output,
    `check()` asserts that the GUARD floats on either side still hold the pattern and that the output holds no NaN,
    `untouched()` that nothing at all was written.  skew: the output starts that many elements later (skew = 1: an output that
    is 4-byte but not 8- or 16-byte aligned); the skipped elements belong to the front guard."""

    def __init__(self, name, shape, dev, skew=0):
        self.name, n = name, int(np.prod(shape))
        self.lo = GUARD + skew
        self.raw = torch.full((n + 2 * GUARD + skew,), FILL, dtype=torch.int32, device=dev)
        self.t = self.raw[self.lo:self.lo + n].view(torch.float32).view(shape)

    def ptr(self):
        return self.t.data_ptr()

    def check(self):
        raw = self.raw                                     # (compared where it lives: three flags cross to the host, not the buffer)
        n = raw.numel() - self.lo - GUARD
        assert bool((raw[:self.lo] == FILL).all()), f"{self.name}: written before its first element"
        assert bool((raw[self.lo + n:] == FILL).all()), f"{self.name}: written past its last element"
        assert not bool(torch.isnan(self.t).any()), f"{self.name}: elements left unwritten (or NaN)"

    def untouched(self):
        assert bool((self.raw == FILL).all().cpu()), f"{self.name}: written by a refused call"


class GuardedWords(GuardedBuffer):
    """The integer variant (shape, int32 holding uint32 bit patterns): sign words, packed weight panels.  `check()` asserts the
    guards and that no word of the output still holds the fill pattern (first: only that many leading words must be written)."""

    def __init__(self, name, shape, dev, skew=0):
        super().__init__(name, shape, dev, skew)
        self.t = self.t.view(torch.int32)

    def check(self, first=None):
        raw = self.raw
        n = raw.numel() - self.lo - GUARD
        assert bool((raw[:self.lo] == FILL).all()), f"{self.name}: written before its first word"
        assert bool((raw[self.lo + n:] == FILL).all()), f"{self.name}: written past its last word"
        body = raw[self.lo:self.lo + (n if first is None else first)]
        assert not bool((body == FILL).any()), f"{self.name}: words left unwritten"
