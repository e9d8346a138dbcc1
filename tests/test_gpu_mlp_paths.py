"""Every launch path of the field networks' C entry points (d3ga_amd/csrc/mlp.hip, include/d3ga.h "Field networks"), called
through d3ga_amd._lib.lib() with raw pointers, against float64 (tests/mlp_ref.py):
  A  d3ga_mlp_pack_weights + d3ga_mlp_linear: a table that reaches every instantiation linear_kernel<NB, VEC, EMASK, RAGGED>
     (the row ids name them: NB1..4, v|s = K % 4 == 0 or not, m|- = mask_bits or not, F|R = the unchecked rows [0, P - P % 32) or the
     bounds-checked rest), the prefix property across that split, and weights packed from strided / transposed / edited storage;
  B  second trips: the per-layer kernel's second tile per workgroup (P > 131072) and the weight gradient's multi-chunk walk;
  C  d3ga_mlp_wgrad / d3ga_mlp_wgrad_acc over every loader layout, under wgrad_ws = 0, 1, 2, aligned and 4-byte aligned;
  D  d3ga_mlp_pack_chain + d3ga_mlp_chain_fwd: a pairwise cover of depth, first and last width, bias, slopes, sign output and the
     alignment of X, forward and the backward's input-gradient chain, with the grid capped (chain_grid = 1, 2, 3) so that every
     workgroup walks several row blocks at a few hundred rows: bit-identical to the default grid;
  E  every refusal of the nine d3ga_mlp_* entry points: the status, and nothing written.
Every output and every panel sits in a guard band (cage_ref.GuardedBuffer / GuardedWords); every pointer, also of a call that
must be refused, is backed by device memory of the declared size.
Bars (the ones tests/test_gpu_mlp.py holds the wrappers to): a single layer |dev - f64| <= 1e-5 |f64| + 1e-5, trunks 2e-5 |f64| +
2e-5, weight / bias gradients up to 1100 rows 1e-5 of max|f64| (max-norm); the multi-chunk weight gradients of B
max(1e-5, 4 e32) of max|f64| with e32 = the error of torch's float32 CPU product against float64 (same precision, another
summation order: the factor 4 of tests/test_gpu_perceptual.py).  Everything called bit-exact is torch.equal."""
import contextlib
import ctypes
import os

import pytest
import torch

import cage_ref as cr
import mlp_ref as mr
from d3ga_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_NULL, E_SIZE, E_CONFIG = -1, -2, -3            # D3GA_E_* (include/d3ga.h)
MASK_SLOPE = 0.3                                 # unlike every out_slope used here
i32 = ctypes.c_int32


def L():
    return _lib.lib()


def S():
    return _lib.stream_handle()


def vp(x):
    """c_void_p of a tensor, a guarded buffer, an address or None."""
    if x is None:
        return None
    if isinstance(x, cr.GuardedBuffer):
        return ctypes.c_void_p(x.ptr())
    return ctypes.c_void_p(x if isinstance(x, int) else x.data_ptr())


def dev_in(t, skew=0):
    """Device copy of an input; skew = 1: it starts 4 bytes into its (256-byte aligned) allocation."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=DEV)
    v = buf[skew:skew + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * skew
    return v


def rand_words(g, P, nw):
    """Random uint32 words (as int32), all 32 bits used: bits past the width must be ignored."""
    return torch.randint(-2 ** 31, 2 ** 31, (P, nw), generator=g, dtype=torch.int64).to(torch.int32)


@contextlib.contextmanager
def knob(name, value):
    """A debug knob of the library for the duration of the block (None: the library as it is, no knob touched)."""
    if value is None:
        yield
        return
    if os.environ.get("D3GA_KNOBS"):
        pytest.skip("D3GA_KNOBS set: the knob under test is the caller's")
    _lib.debug_set(name, value)
    try:
        yield
    finally:
        _lib.debug_set(name)


def assert_bar(got, ref, rel, tag):
    """|got - ref| <= rel |ref| + rel, element-wise."""
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    if ref.numel() == 0:
        return
    over = ((got - ref).abs() - (rel * ref.abs() + rel)).max().item()
    assert over <= 0.0, f"{tag}: {over:.3e} above the bar {rel:g} |f64| + {rel:g} (max |diff| {(got - ref).abs().max().item():.3e})"


def max_norm_err(got, ref):
    return ((got.detach().cpu().double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


# ----------------------------------------------------------------------------------------------------------------------------
# A. d3ga_mlp_pack_weights + d3ga_mlp_linear
# ----------------------------------------------------------------------------------------------------------------------------
def pack_linear(K, N, W, ld_k, ld_n, into=None):
    """d3ga_mlp_pack_weights into a guarded panel (checked: guards intact, every word written)."""
    nbytes = L().d3ga_mlp_panel_bytes(K, N)
    assert nbytes == 16 * 3 * ((K + 15) // 16) * 2 * mr.n_words(N) * 32
    p = into if into is not None else cr.GuardedWords(f"panel K{K} N{N}", (nbytes // 4,), DEV)
    assert L().d3ga_mlp_pack_weights(K, N, vp(W), ld_k, ld_n, vp(p), S()) == 0
    torch.cuda.synchronize()
    p.check()
    return p


def pack_linear_kn(Wkn):
    """The panel of Wkn (K, N) from its nn.Linear layout (N, K): ld_k = 1, ld_n = K."""
    K, N = Wkn.shape
    return pack_linear(K, N, dev_in(Wkn.T.contiguous()), 1, K)


def run_linear(P, K, N, x, panel, bias, slope, want_sign, mask=None, mask_slope=1.0):
    """One d3ga_mlp_linear call into guarded outputs -> (Y, sign words or None), guards checked."""
    Y = cr.GuardedBuffer(f"Y P{P} K{K} N{N}", (P, N), DEV)
    sg = cr.GuardedWords(f"sign_out P{P} N{N}", (P, mr.n_words(N)), DEV) if want_sign else None
    st = L().d3ga_mlp_linear(P, K, N, vp(x), vp(panel), vp(bias), float(slope), vp(sg), vp(mask), float(mask_slope), vp(Y), S())
    assert st == 0, st
    torch.cuda.synchronize()
    Y.check()
    if sg is not None:
        sg.check()
    panel.check()
    return Y, sg


def prefix_points(P):
    """Row counts p < P whose call must reproduce rows [0, p) of the P-row call: one less, the end of the unchecked part, half."""
    return sorted({p for p in (P - 1, P - P % 32, P // 2, 1) if 0 < p < P})


LIN_ROWS = mr.linear_table()


def test_linear_table_covers_every_instantiation_and_pair():
    """The table itself: all 32 instantiations, every pair of factor values, and rows that have sign or mask words on both sides
    of the full / rest split with more than one word per row (the word offset `wo` of the launcher)."""
    assert {x for r in LIN_ROWS for x in r["inst"]} == mr.ALL_LINEAR_INSTANCES
    factors = dict(n_out=mr.LIN_NOUT, K=mr.LIN_K, P=mr.LIN_P, mask=(False, True), sign=(False, True), bias=(False, True), slope=(1.0, 0.1))
    assert mr.pairs_missing(LIN_ROWS, factors) == []
    split_words = [r for r in LIN_ROWS if len(r["inst"]) == 2 and r["n_out"] > 32 and (r["sign"] or r["mask"])]
    assert any(r["sign"] for r in split_words) and any(r["mask"] for r in split_words), [r["id"] for r in split_words]


@pytest.mark.parametrize("row", LIN_ROWS, ids=[r["id"] for r in LIN_ROWS])
def test_linear_instantiation(row):
    """One row of the table: values against float64, sign words against the kernel's own Y > 0, the masked output against the
    unmasked one times (bit ? 1 : mask_slope) in float32, guards, and the prefix property (a row's arithmetic does not depend on
    its neighbours, so the p-row call equals rows [0, p) of the P-row call bit for bit, across both instantiations)."""
    P, K, N = row["P"], row["K"], row["n_out"]
    g = torch.Generator().manual_seed(1000 + LIN_ROWS.index(row))
    x, Wkn = torch.randn(P, K, generator=g), torch.randn(K, N, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g) if row["bias"] else None
    mw = rand_words(g, P, mr.n_words(N))
    xd, bd, mwd = dev_in(x), (dev_in(b) if b is not None else None), dev_in(mw)
    panel = pack_linear_kn(Wkn)
    ref = mr.dense(x, Wkn, b, row["slope"])
    Y0, s0 = run_linear(P, K, N, xd, panel, bd, row["slope"], row["sign"])
    y0 = Y0.t.cpu()
    assert_bar(y0, ref, 1e-5, "Y")
    if row["sign"]:
        assert torch.equal(s0.t.cpu(), mr.pack_signs(y0 > 0)), "sign words differ from the kernel's own Y > 0"
    runs = [(None, Y0, s0)]
    if row["mask"]:
        Ym, sm = run_linear(P, K, N, xd, panel, bd, row["slope"], row["sign"], mwd, MASK_SLOPE)
        keep = mr.unpack_signs(mw, N)
        assert torch.equal(Ym.t.cpu(), y0 * mr.mask_factor(keep, MASK_SLOPE, torch.float32)), "masked output is not Y (.) (bit ? 1 : mask_slope)"
        assert_bar(Ym.t, ref * mr.mask_factor(keep, MASK_SLOPE), 1e-5, "masked Y")
        if row["sign"]:
            assert torch.equal(sm.t.cpu(), mr.pack_signs(Ym.t.cpu() > 0))
        runs.append((mwd, Ym, sm))
    for p in prefix_points(P):
        for mask, Yf, sf in runs:
            Yp, sp = run_linear(p, K, N, xd, panel, bd, row["slope"], row["sign"], mask, MASK_SLOPE)
            assert torch.equal(Yp.t, Yf.t[:p]), f"rows [0, {p}) of the {P}-row call differ from the {p}-row call"
            if row["sign"]:
                assert torch.equal(sp.t, sf.t[:p]), f"sign words of rows [0, {p}) differ between the {P}- and the {p}-row call"


PACK_SHAPES = [(11, 33), (128, 128), (17, 97), (4, 1), (48, 64)]


@pytest.mark.parametrize("chain", [False, True], ids=["linear", "chain"])
@pytest.mark.parametrize("K,N", PACK_SHAPES)
def test_pack_from_strided_transposed_and_edited_weights(K, N, chain):
    """d3ga_mlp_pack_weights / d3ga_mlp_pack_chain read weight(k, n) = W[k ld_k + n ld_n]: the same matrix as an nn.Linear weight
    (ld_k = 1, ld_n = K), transposed (the input-gradient GEMM's layout: ld_k = row length, ld_n = 1), as every second column of a
    wider array and as the inside of a larger transposed one gives the same panel bit for bit; a re-pack after an in-place edit of
    the weights equals the pack of a fresh copy and differs from the old panel."""
    g = torch.Generator().manual_seed(7 * K + N)
    Wkn = torch.randn(K, N, generator=g) / K ** 0.5
    n_bytes = (L().d3ga_mlp_chain_panel_bytes if chain else L().d3ga_mlp_panel_bytes)(K, N)
    body = n_bytes // 4 - (128 if chain else 0)            # (the chain panel's 512-byte tail belongs to d3ga_mlp_chain_fwd)
    fn = L().d3ga_mlp_pack_chain if chain else L().d3ga_mlp_pack_weights

    def pack(W, ld_k, ld_n, into=None):
        p = into if into is not None else cr.GuardedWords("panel", (n_bytes // 4,), DEV)
        assert fn(K, N, vp(W), ld_k, ld_n, vp(p), S()) == 0
        torch.cuda.synchronize()
        p.check(first=body)
        return p
    w_nk = dev_in(Wkn.T.contiguous())
    base = pack(w_nk, 1, K)
    if chain:
        assert bool((base.t[body:] == cr.FILL).all()), "d3ga_mlp_pack_chain wrote the bias tail"
    w_kn = dev_in(Wkn)
    assert torch.equal(pack(w_kn, N, 1).t[:body], base.t[:body]), "transposed layout"
    wide = torch.full((N, 2 * K + 3), float("nan"), device=DEV)
    wide[:, 1:2 * K + 1:2] = Wkn.T.to(DEV)
    assert torch.equal(pack(wide[:, 1:], 2, 2 * K + 3).t[:body], base.t[:body]), "every second column of a wider array"
    big = torch.full((K + 2, N + 5), float("nan"), device=DEV)
    big[1:K + 1, 2:N + 2] = Wkn.to(DEV)
    assert torch.equal(pack(big[1:, 2:], N + 5, 1).t[:body], base.t[:body]), "the inside of a larger transposed array"
    old = base.t.clone()
    w_nk.mul_(-1.5).add_(0.25)
    pack(w_nk, 1, K, into=base)
    assert torch.equal(base.t[:body], pack(w_nk.clone(), 1, K).t[:body]), "re-pack after an in-place edit"
    assert not torch.equal(base.t[:body], old[:body])


def test_linear_input_gradient_layout_matches_f64():
    """The header's input-gradient GEMM: from an nn.Linear weight (n_layer, k_layer), K := n_layer, n_out := k_layer, ld_k = k_layer,
    ld_n = 1, with the sign words of the layer below as mask -> dPre of that layer."""
    n_layer, k_layer, P = 33, 100, 77
    g = torch.Generator().manual_seed(5)
    W = torch.randn(n_layer, k_layer, generator=g) / k_layer ** 0.5
    dpre, mw = torch.randn(P, n_layer, generator=g), rand_words(g, P, mr.n_words(k_layer))
    panel = pack_linear(n_layer, k_layer, dev_in(W), k_layer, 1)
    Y, _ = run_linear(P, n_layer, k_layer, dev_in(dpre), panel, None, 1.0, False, dev_in(mw), 0.1)
    assert_bar(Y.t, (dpre.double() @ W.double()) * mr.mask_factor(mr.unpack_signs(mw, k_layer), 0.1), 1e-5, "dPre below")


# ----------------------------------------------------------------------------------------------------------------------------
# B. second trips
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [128, 11])
def test_linear_second_tile_per_workgroup(N):
    """P = 131072 + 512 + 17 rows: 258 tiles of 512 rows over a grid of 256 workgroups, so two workgroups take a second tile (with
    the first tile's last prefetch aimed at it); at N = 128 the unchecked instantiation does that and 17 rows go to the checked one,
    at N = 11 the checked one walks all of it.  Rows [131072, P) bit for bit against a call on X[131072:], 4096 sampled rows
    against float64."""
    P, K, cut = 131072 + 512 + 17, 128, 131072
    g = torch.Generator().manual_seed(N)
    x, Wkn, b = torch.randn(P, K, generator=g), torch.randn(K, N, generator=g) / K ** 0.5, torch.randn(N, generator=g)
    xd, bd, panel = dev_in(x), dev_in(b), pack_linear_kn(Wkn)
    Y, sg = run_linear(P, K, N, xd, panel, bd, 0.1, True)
    Yt, st = run_linear(P - cut, K, N, xd[cut:], panel, bd, 0.1, True)
    assert torch.equal(Y.t[cut:], Yt.t) and torch.equal(sg.t[cut:], st.t)
    rows = torch.cat([torch.randperm(P, generator=g)[:4096 - 600], torch.arange(P - 600, P)])
    y = Y.t.cpu()
    assert_bar(y[rows], mr.dense(x[rows], Wkn, b, 0.1), 1e-5, "sampled rows")
    assert torch.equal(sg.t.cpu()[rows], mr.pack_signs(y[rows] > 0))


def run_wgrad(acc, P, N, K, dpre, x, dW, db):
    fn = L().d3ga_mlp_wgrad_acc if acc else L().d3ga_mlp_wgrad
    st = fn(P, N, K, vp(dpre), vp(x), vp(dW), vp(db), S())
    torch.cuda.synchronize()
    return st


@pytest.mark.parametrize("ws", [None, 0, 2], ids=["ws_default", "ws0", "ws2"])
@pytest.mark.parametrize("N,K", [(128, 128), (11, 128), (128, 3)])
@pytest.mark.parametrize("P", [16384 + 64 + 5, 40001])
def test_wgrad_multi_chunk_walk(P, N, K, ws):
    """More than 16384 rows: every workgroup of the weight gradient walks several chunks of its row range (a ragged last one
    included).  Bar: max(1e-5, 4 e32) of max|f64|, e32 = torch's float32 CPU product of the same operands against float64."""
    g = torch.Generator().manual_seed(P + N + K)
    dpre, x = torch.randn(P, N, generator=g), torch.randn(P, K, generator=g)
    rW, rb = mr.wgrad(dpre, x)
    e32W, e32b = max_norm_err(dpre.T @ x, rW), max_norm_err(dpre.sum(0), rb)
    dW, db = cr.GuardedBuffer("dW", (N, K), DEV), cr.GuardedBuffer("db", (N,), DEV)
    with knob("wgrad_ws", ws):
        assert run_wgrad(False, P, N, K, dev_in(dpre), dev_in(x), dW, db) == 0
    dW.check()
    db.check()
    eW, eb = max_norm_err(dW.t, rW), max_norm_err(db.t, rb)
    print(f"wgrad P={P} N={N} K={K} ws={ws}: dW e32 {e32W:.3e} device {eW:.3e} | db e32 {e32b:.3e} device {eb:.3e}")
    assert eW <= max(1e-5, 4.0 * e32W) and eb <= max(1e-5, 4.0 * e32b), (eW, e32W, eb, e32b)


# ----------------------------------------------------------------------------------------------------------------------------
# C. d3ga_mlp_wgrad and d3ga_mlp_wgrad_acc
# ----------------------------------------------------------------------------------------------------------------------------
WG_SHAPES = {  # (N, K)
    "wide_wide": [(128, 128), (64, 96)], "narrowN_wideK": [(11, 128), (16, 64), (1, 97), (4, 33)],
    "wideN_narrowK": [(128, 3), (65, 16), (32, 1)], "narrow_narrow": [(11, 3), (16, 16), (1, 1), (2, 4)],
    "odd": [(33, 65), (97, 127), (17, 31)], "block_edges": [(32, 33), (33, 32), (64, 65), (65, 64), (96, 97), (97, 96)]}
WG_LIST = [(k, nk) for k, v in WG_SHAPES.items() for nk in v]
WG_IDS = [f"{k}_N{n}_K{kk}" for k, (n, kk) in WG_LIST]
WG_P = (1, 7, 8, 9, 31, 33, 63, 64, 65, 1000)
WG_EVEN = [(k, (n, kk)) for k, (n, kk) in WG_LIST if n % 2 == 0 and kk % 2 == 0] + [("even", (18, 34)), ("even", (34, 128)), ("even", (128, 2))]


def wgrad_inputs(N, K, Ps):
    """dPre, X ~ N(0,1) for the largest row count (every smaller one takes a prefix) and the dW / db the accumulating form starts
    from.  The bar is relative to the LARGEST element of the float64 result; with one or two columns that can be a single sum that
    happens to cancel (N = 1, 33 rows: 33 terms of sum |t| = 25.7 meeting in 0.023, where torch's own float32 sum is 1.1e-5 off
    and a sequential one 3.3e-5), and then no float32 summation meets 1e-5.  Decided on the CPU, without the code under test: a
    draw is taken only if torch's float32 evaluation stays within a quarter of the bar at every row count (the rule of part B,
    4 e32 <= bar), else the next seed is drawn."""
    Pm = max(Ps)
    for attempt in range(16):
        g = torch.Generator().manual_seed(100 * N + K + 100000 * attempt)
        dpre, x = torch.randn(Pm, N, generator=g), torch.randn(Pm, K, generator=g)
        W0, b0 = torch.randn(N, K, generator=g), torch.randn(N, generator=g)
        e32 = 0.0
        for P in Ps:
            rW, rb = mr.wgrad(dpre[:P], x[:P])
            e32 = max(e32, max_norm_err(dpre[:P].T @ x[:P], rW), max_norm_err(dpre[:P].sum(0), rb),
                      max_norm_err(W0 + dpre[:P].T @ x[:P], W0.double() + rW), max_norm_err(b0 + dpre[:P].sum(0), b0.double() + rb))
        if 4.0 * e32 <= 1e-5:
            return dpre, x, W0, b0
    raise AssertionError(f"no well-conditioned draw for N={N} K={K}")


def wgrad_contracts(N, K, ws, skew, Ps):
    dpre, x, W0, b0 = wgrad_inputs(N, K, Ps)
    Pm = max(Ps)
    with knob("wgrad_ws", ws):
        for P in Ps:
            # (a prefix of the rows, re-laid at the wanted alignment)
            dd, xx = dev_in(dpre[:P].contiguous(), skew), dev_in(x[:P].contiguous(), skew)
            rW, rb = mr.wgrad(dpre[:P], x[:P])
            for acc in (False, True):
                dW, db = cr.GuardedBuffer("dW", (N, K), DEV, skew), cr.GuardedBuffer("db", (N,), DEV)
                if acc:                                    # adds to what is there
                    dW.t.copy_(W0)
                    db.t.copy_(b0)
                assert run_wgrad(acc, P, N, K, dd, xx, dW, db) == 0
                dW.check()                                 # (zeroing form: the NaN fill is gone, so it overwrote)
                db.check()
                wantW, wantb = (rW + W0.double(), rb + b0.double()) if acc else (rW, rb)
                eW, eb = max_norm_err(dW.t, wantW), max_norm_err(db.t, wantb)
                assert eW <= 1e-5 and eb <= 1e-5, (P, N, K, "acc" if acc else "zeroing", eW, eb)
        # db = NULL is accepted, and dW is the same sum
        P = Ps[len(Ps) // 2]
        dd, xx = dev_in(dpre[:P].contiguous(), skew), dev_in(x[:P].contiguous(), skew)
        dW = cr.GuardedBuffer("dW", (N, K), DEV, skew)
        assert run_wgrad(False, P, N, K, dd, xx, dW, None) == 0
        dW.check()
        assert max_norm_err(dW.t, mr.wgrad(dpre[:P], x[:P])[0]) <= 1e-5
        # P = 0: the zeroing form zeroes, the accumulating form writes nothing
        dW, db = cr.GuardedBuffer("dW", (N, K), DEV, skew), cr.GuardedBuffer("db", (N,), DEV)
        assert run_wgrad(True, 0, N, K, dd, xx, dW, db) == 0
        dW.untouched()
        db.untouched()
        assert run_wgrad(False, 0, N, K, dd, xx, dW, db) == 0
        dW.check()
        db.check()
        assert float(dW.t.abs().sum()) == 0.0 and float(db.t.abs().sum()) == 0.0


@pytest.mark.parametrize("ws", [0, 1, 2])
@pytest.mark.parametrize("shape", WG_LIST, ids=WG_IDS)
def test_wgrad_every_layout(shape, ws):
    """Both forms over the loader layouts of the two kernels (two wide operands; a narrow dPre; a narrow X; both narrow; odd widths;
    widths at the 32-column block edges), row counts around the 8-row group, the 32- and 64-row chunk, under each routing of
    wgrad_ws (0: the barrier-phased kernel everywhere, wgrad_kernel<., ., false> for two wide operands; 1: the default; 2: the
    wavefront-specialised kernel for every shape).  Each run against float64 (the summation orders differ between the routings)."""
    wgrad_contracts(*shape[1], ws, 0, WG_P)


@pytest.mark.parametrize("ws", [0, 1, 2])
@pytest.mark.parametrize("shape", WG_EVEN, ids=[f"{k}_N{n}_K{kk}" for k, (n, kk) in WG_EVEN])
def test_wgrad_four_byte_aligned_operands(shape, ws):
    """dPre, X and dW 4 bytes into their buffers, even widths: the launcher must not take the 8-byte loads (va / vb false)."""
    wgrad_contracts(*shape[1], ws, 1, (1, 9, 33, 64, 65, 1000))


# ----------------------------------------------------------------------------------------------------------------------------
# D. d3ga_mlp_pack_chain + d3ga_mlp_chain_fwd
# ----------------------------------------------------------------------------------------------------------------------------
def pack_chain(K, N, W, ld_k, ld_n):
    nbytes = L().d3ga_mlp_chain_panel_bytes(K, N)
    assert nbytes == 16 * 3 * 2 * ((K + 31) // 32) * mr.n_words(N) * 64 + 512
    p = cr.GuardedWords(f"chain panel K{K} N{N}", (nbytes // 4,), DEV)
    assert L().d3ga_mlp_pack_chain(K, N, vp(W), ld_k, ld_n, vp(p), S()) == 0
    torch.cuda.synchronize()
    p.check(first=nbytes // 4 - 128)
    return p


def c_arr(ctype, vals, n=None):
    vals = list(vals)
    return (ctype * (n or len(vals)))(*vals)


def ptr_arr(items, n=None):
    """void *[]: tensors / guarded buffers / addresses / None."""
    items = list(items)
    a = (ctypes.c_void_p * (n or len(items)))()
    for k, it in enumerate(items):
        v = vp(it)
        a[k] = None if v is None else v.value
    return a


def run_chain(P, x, dims, panels, biases, slopes, want_signs, masks=None, mask_slopes=None, tails_written=True):
    """One d3ga_mlp_chain_fwd call into guarded outputs -> (outs, signs), every guard checked (panels too)."""
    Ln = len(dims)
    outs = [cr.GuardedBuffer(f"outs[{l}]", (P, n), DEV) for l, (_, n) in enumerate(dims)]
    signs = [cr.GuardedWords(f"signs[{l}]", (P, mr.n_words(n)), DEV) if w else None for l, ((_, n), w) in enumerate(zip(dims, want_signs))]
    st = L().d3ga_mlp_chain_fwd(P, dims[0][0], vp(x), Ln, c_arr(i32, [k for k, _ in dims]), c_arr(i32, [n for _, n in dims]),
                                ptr_arr(panels), None if biases is None else ptr_arr(biases), c_arr(ctypes.c_float, slopes),
                                ptr_arr(outs), ptr_arr(signs), None if masks is None else ptr_arr(masks),
                                None if mask_slopes is None else c_arr(ctypes.c_float, mask_slopes), S())
    assert st == 0, st
    torch.cuda.synchronize()
    for b in outs + [s for s in signs if s is not None]:
        b.check()
    for p in panels:
        p.check(first=None if tails_written else p.t.numel() - 128)
    return outs, signs


CHAIN_ROWS_T = mr.chain_table()
_PMAX = max(mr.CHAIN_ROWS)


def test_chain_table_is_a_pairwise_cover():
    factors = dict(L=mr.CHAIN_L, K0=mr.CHAIN_K0, last=mr.CHAIN_LAST, bias=mr.CHAIN_BIAS, slopes=mr.CHAIN_SLOPES, signs=(False, True),
                   xoff=(False, True))
    assert mr.pairs_missing(CHAIN_ROWS_T, factors) == []
    assert {r["nch0"] for r in CHAIN_ROWS_T} == {1, 2, 3, 4} and {r["ntl"] for r in CHAIN_ROWS_T} == {1, 2, 3, 4}


@pytest.fixture(scope="module", params=CHAIN_ROWS_T, ids=[r["id"] for r in CHAIN_ROWS_T])
def chain_case(request):
    """A row of the table: weights, biases, inputs (CPU), the float64 trunk on all 1281 rows (a prefix of it is the reference of
    every smaller row count: rows are independent), device copies and the packed panels of the forward and of the backward."""
    r = request.param
    g = torch.Generator().manual_seed(2000 + CHAIN_ROWS_T.index(r))
    widths = [r["K0"]] + [128] * (r["L"] - 1) + [r["last"]]
    dims = list(zip(widths[:-1], widths[1:]))
    Ws = [torch.randn(k, n, generator=g) / k ** 0.5 for k, n in dims]
    bs = [torch.randn(n, generator=g) for _, n in dims]
    if r["bias"] == "absent":
        bs = None
    elif r["bias"] == "some":
        bs = [b if l % 2 == 0 else None for l, b in enumerate(bs)]
    slopes = [r["slopes"][0]] * (r["L"] - 1) + [r["slopes"][1]]
    x = torch.randn(_PMAX, r["K0"], generator=g)
    ref = mr.trunk_forward(x, [(W, None if bs is None else bs[l]) for l, W in enumerate(Ws)], slopes)
    c = dict(row=r, dims=dims, Ws=Ws, bs=bs, slopes=slopes, x=x, ref=ref, up=torch.randn(_PMAX, r["last"], generator=g))
    c["bs_d"] = None if bs is None else [None if b is None else dev_in(b) for b in bs]
    c["panels"] = [pack_chain(k, n, dev_in(W.T.contiguous()), 1, k) for (k, n), W in zip(dims, Ws)]
    c["snap"] = [p.t.clone() for p in c["panels"]]
    # the backward's chain: call layer j = model layer L - 1 - j transposed (from the model's (K, N) array: ld_k = 1, ld_n = N)
    c["bdims"] = [(n, k) for k, n in reversed(dims)]
    c["bpanels"] = [pack_chain(n, k, dev_in(W), 1, n) for (k, n), W in zip(reversed(dims), reversed(Ws))]
    return c


def chain_forward(c, P, want_signs=None):
    r = c["row"]
    xd = dev_in(c["x"][:P].contiguous(), 1 if r["xoff"] else 0)
    ws = [r["signs"]] * r["L"] if want_signs is None else want_signs
    return run_chain(P, xd, c["dims"], c["panels"], c["bs_d"], c["slopes"], ws)


def assert_same(a, b, tag):
    for l, (u, v) in enumerate(zip(a, b)):
        assert (u is None) == (v is None)
        if u is not None:
            assert torch.equal(u.t, v.t), f"{tag}: layer {l} differs"


def test_chain_forward_against_f64(chain_case):
    """Every layer's output against the float64 trunk (2e-5 |f64| + 2e-5), every sign word against the kernel's own output > 0
    (the slopes here are positive, so out > 0 is pre-activation > 0), at the four row counts; the panels' weight parts are left as
    d3ga_mlp_pack_chain wrote them and their tails hold this call's biases (zeros past the width and for a NULL bias); a second call
    with no biases at all leaves zeros there and the weights alone."""
    c = chain_case
    for P in mr.CHAIN_ROWS:
        outs, signs = chain_forward(c, P)
        for l, o in enumerate(outs):
            assert_bar(o.t, c["ref"][l][:P], 2e-5, f"P={P} outs[{l}]")
            if signs[l] is not None:
                assert torch.equal(signs[l].t.cpu(), mr.pack_signs(o.t.cpu() > 0)), f"P={P} signs[{l}]"
        for l, (p, snap) in enumerate(zip(c["panels"], c["snap"])):
            assert torch.equal(p.t[:-128], snap[:-128]), f"panel {l}: weights changed by the forward"
            want = torch.zeros(128)
            if c["bs"] is not None and c["bs"][l] is not None:
                want[:c["dims"][l][1]] = c["bs"][l]
            assert torch.equal(p.t[-128:].view(torch.float32).cpu(), want), f"panel {l}: tail is not this call's bias"
    # another bias (none) through the same panels
    P = mr.CHAIN_ROWS[0]
    xd = dev_in(c["x"][:P].contiguous())
    outs, _ = run_chain(P, xd, c["dims"], c["panels"], None, c["slopes"], [False] * len(c["dims"]))
    ref0 = mr.trunk_forward(c["x"][:P], [(W, None) for W in c["Ws"]], c["slopes"])
    assert_bar(outs[-1].t, ref0[-1], 2e-5, "no bias")
    for l, (p, snap) in enumerate(zip(c["panels"], c["snap"])):
        assert torch.equal(p.t[:-128], snap[:-128]) and float(p.t[-128:].view(torch.float32).abs().sum()) == 0.0, f"panel {l}"


def chain_backward_args(c, P, fsigns, drop_some):
    """masks / mask slopes of the backward's chain from the forward's sign words: call layer j (model layer i = L - 1 - j) is masked
    by the words of model layer i - 1; its last layer (i = 0) has none.  drop_some: masks[j] = NULL on every other layer."""
    r, Ln = c["row"], c["row"]["L"]
    masks, ms = [], []
    for j in range(Ln):
        i = Ln - 1 - j
        masks.append(fsigns[i - 1] if i > 0 and not (drop_some and j % 2 == 1) else None)
        ms.append(MASK_SLOPE if r["slopes"][0] == 1.0 else r["slopes"][0])
    return masks, ms


def chain_backward_ref(c, P, masks, ms):
    mats = [W.T for W in reversed(c["Ws"])]
    bits = [None if m is None else mr.unpack_signs(m.t, 128) for m in masks]
    return mr.chain_backward(c["up"][:P], mats, bits, ms)


@pytest.mark.parametrize("drop_some", [False, True], ids=["all_masks", "some_masks_null"])
def test_chain_backward_against_f64(chain_case, drop_some):
    """The backward's input-gradient chain through the same launch: transposed panels, masks = the sign words the forward wrote,
    mask slopes; every layer's output (the pre-activation gradients, then dX) against the header's definition in float64."""
    c = chain_case
    Ln = c["row"]["L"]
    for P in mr.CHAIN_ROWS[:2] if drop_some else mr.CHAIN_ROWS:
        _, fsigns = chain_forward(c, P, [True] * Ln)
        masks, ms = chain_backward_args(c, P, fsigns, drop_some)
        outs, _ = run_chain(P, dev_in(c["up"][:P].contiguous()), c["bdims"], c["bpanels"], None, [1.0] * Ln, [False] * Ln, masks, ms,
                            tails_written=False)
        for l, (o, ref) in enumerate(zip(outs, chain_backward_ref(c, P, masks, ms))):
            assert_bar(o.t, ref, 2e-5, f"P={P} backward outs[{l}]")


def test_chain_grid_cap_is_bit_identical(chain_case):
    """chain_grid = 1, 2, 3: one to three workgroups walk all the row blocks (up to six each, a ragged last block, an uneven split),
    prefetching the next block's first chunk and bias during their last layer, with the slot parity and the bias buffers carried
    from block to block.  Forward (outputs and sign words) and backward chain bit for bit equal to the default grid's."""
    c = chain_case
    Ln = c["row"]["L"]
    for P in mr.CHAIN_ROWS:
        outs, signs = chain_forward(c, P, [True] * Ln)
        masks, ms = chain_backward_args(c, P, signs, False)
        up = dev_in(c["up"][:P].contiguous())
        bouts, _ = run_chain(P, up, c["bdims"], c["bpanels"], None, [1.0] * Ln, [False] * Ln, masks, ms, tails_written=False)
        for grid in (1, 2, 3):
            with knob("chain_grid", grid):
                o2, s2 = chain_forward(c, P, [True] * Ln)
                b2, _ = run_chain(P, up, c["bdims"], c["bpanels"], None, [1.0] * Ln, [False] * Ln, masks, ms, tails_written=False)
            assert_same(o2, outs, f"P={P} chain_grid={grid} forward")
            assert_same(s2, signs, f"P={P} chain_grid={grid} sign words")
            assert_same(b2, bouts, f"P={P} chain_grid={grid} backward")


def test_chain_without_mask_array_runs_the_forward_instantiation():
    """masks = NULL with no bias, slopes 1 and no sign output is still the forward instantiation (zero bias from the tails): the same
    products as the backward one, so both agree with float64 and with each other bit for bit."""
    g = torch.Generator().manual_seed(9)
    P, dims = 300, [(40, 128), (128, 128), (128, 7)]
    Ws = [torch.randn(k, n, generator=g) / k ** 0.5 for k, n in dims]
    x = torch.randn(P, 40, generator=g)
    panels = [pack_chain(k, n, dev_in(W), n, 1) for (k, n), W in zip(dims, Ws)]
    xd = dev_in(x)
    fwd, _ = run_chain(P, xd, dims, panels, None, [1.0] * 3, [False] * 3)
    bwd, _ = run_chain(P, xd, dims, panels, None, [1.0] * 3, [False] * 3, [None] * 3, None)
    ref = mr.trunk_forward(x, [(W, None) for W in Ws], [1.0] * 3)
    for l in range(3):
        assert_bar(fwd[l].t, ref[l], 2e-5, f"outs[{l}]")
    assert_same(fwd, bwd, "forward against backward instantiation")


# ----------------------------------------------------------------------------------------------------------------------------
# E. refusals: the status, and nothing written
# ----------------------------------------------------------------------------------------------------------------------------
class Frozen:
    """Snapshots of guarded buffers (bands included): `same()` asserts that a call wrote nothing into any of them."""

    def __init__(self, *bufs):
        torch.cuda.synchronize()
        self.bufs = [b for b in bufs if b is not None]
        self.snap = [b.raw.clone() for b in self.bufs]

    def same(self, tag):
        torch.cuda.synchronize()
        for b, s in zip(self.bufs, self.snap):
            assert torch.equal(b.raw, s), f"{tag}: {b.name} written by a refused call"


def test_panel_bytes_refusals():
    for fn in (L().d3ga_mlp_panel_bytes, L().d3ga_mlp_chain_panel_bytes):
        for K, N in ((0, 8), (129, 8), (8, 0), (8, 129), (-1, 8), (8, -1)):
            assert fn(K, N) == E_SIZE, (K, N)
        assert fn(1, 1) > 0 and fn(128, 128) > 0


@pytest.mark.parametrize("chain", [False, True], ids=["pack_weights", "pack_chain"])
def test_pack_refusals(chain):
    fn = L().d3ga_mlp_pack_chain if chain else L().d3ga_mlp_pack_weights
    nbytes = (L().d3ga_mlp_chain_panel_bytes if chain else L().d3ga_mlp_panel_bytes)(128, 128)
    panel = cr.GuardedWords("panel", (nbytes // 4 + 8,), DEV)           # (room for K, N = 128 and for the 4-byte shift)
    W = torch.randn(129, 129, device=DEV)
    fz = Frozen(panel)
    for K, N, want in ((0, 8, E_SIZE), (129, 8, E_SIZE), (8, 0, E_SIZE), (8, 129, E_SIZE)):
        assert fn(K, N, vp(W), 1, 129, vp(panel), S()) == want, (K, N)
    assert fn(8, 8, None, 1, 8, vp(panel), S()) == E_NULL
    assert fn(8, 8, vp(W), 1, 8, None, S()) == E_NULL
    for shift in (4, 8, 12):
        assert fn(8, 8, vp(W), 1, 8, vp(panel.ptr() + shift), S()) == E_CONFIG
    fz.same("pack")


def test_linear_refusals():
    P, K, N = 40, 12, 33
    x = torch.randn(P + 1, 129, device=DEV)                               # (covers K = 129 and a 4-byte shift)
    Wkn = torch.randn(K, N) / K ** 0.5
    panel_big = cr.GuardedWords("panel", (L().d3ga_mlp_panel_bytes(128, 128) // 4 + 8,), DEV)
    assert L().d3ga_mlp_pack_weights(K, N, vp(dev_in(Wkn)), N, 1, vp(panel_big), S()) == 0
    bias, mask = torch.randn(129, device=DEV), torch.zeros(P, 5, dtype=torch.int32, device=DEV)
    Y, sg = cr.GuardedBuffer("Y", (P, 129), DEV), cr.GuardedWords("sign_out", (P, 5), DEV)
    fz = Frozen(Y, sg, panel_big)

    def call(P=P, K=K, N=N, X=x, pan=panel_big, Yp=Y):
        return L().d3ga_mlp_linear(P, K, N, vp(X), vp(pan), vp(bias), 0.1, vp(sg), vp(mask), 0.5, vp(Yp), S())
    for kw in (dict(P=-1), dict(K=0), dict(K=129), dict(N=0), dict(N=129)):
        assert call(**kw) == E_SIZE, kw
    for kw in (dict(X=None), dict(pan=None), dict(Yp=None)):
        assert call(**kw) == E_NULL, kw
    for kw in (dict(X=x.data_ptr() + 4), dict(X=x.data_ptr() + 8), dict(pan=panel_big.ptr() + 4)):
        assert call(**kw) == E_CONFIG, kw
    assert call(P=0) == 0                                                  # nothing to do is not a refusal, and writes nothing
    assert call(P=0, X=None, pan=None, Yp=None) == 0
    fz.same("d3ga_mlp_linear")
    assert call() == 0                                                     # (the base call of all the above is a valid one)
    torch.cuda.synchronize()


@pytest.mark.parametrize("acc", [False, True], ids=["wgrad", "wgrad_acc"])
def test_wgrad_refusals(acc):
    """Both forms; the zeroing one must refuse BEFORE it zeroes (it used to clear dW / db and then find dpre or X missing)."""
    P, N, K = 40, 12, 33
    dpre, x = torch.randn(P, 129, device=DEV), torch.randn(P, 129, device=DEV)
    dW, db = cr.GuardedBuffer("dW", (129, 129), DEV), cr.GuardedBuffer("db", (129,), DEV)
    fz = Frozen(dW, db)

    def call(P=P, N=N, K=K, d=dpre, X=x, W=dW, b=db):
        return run_wgrad(acc, P, N, K, d, X, W, b)
    for kw in (dict(P=-1), dict(N=0), dict(N=129), dict(K=0), dict(K=129)):
        assert call(**kw) == E_SIZE, kw
    for kw in (dict(W=None), dict(d=None), dict(X=None), dict(d=None, b=None)):
        assert call(**kw) == E_NULL, kw
    fz.same("d3ga_mlp_wgrad" + ("_acc" if acc else ""))
    assert call() == 0


def chain_refusal_scene():
    """A valid 3-layer call (P = 40, 12 -> 128 -> 128 -> 33) with every array sized for L = 9 and every buffer for widths of 129."""
    P, n = 40, 9
    dims = [(12, 128), (128, 128), (128, 33)] + [(33, 33)] * 6
    nb = L().d3ga_mlp_chain_panel_bytes(128, 128) // 4 + 8
    s = dict(P=P, K0=12, L=3, X=torch.randn(P + 1, 129, device=DEV), Ks=[k for k, _ in dims], Ns=[m for _, m in dims],
             panels=[cr.GuardedWords(f"panels[{l}]", (nb,), DEV) for l in range(n)], biases=[torch.randn(129, device=DEV) for _ in range(n)],
             slopes=[0.1, 0.1, 1.0] + [1.0] * 6, outs=[cr.GuardedBuffer(f"outs[{l}]", (P + 1, 129), DEV) for l in range(n)],
             signs=[cr.GuardedWords(f"signs[{l}]", (P + 1, 5), DEV) for l in range(n)], masks=None, mask_slopes=None)
    g = torch.Generator().manual_seed(3)
    for l, (k, m) in enumerate(dims):
        assert L().d3ga_mlp_pack_chain(k, m, vp(dev_in(torch.randn(k, m, generator=g))), m, 1, vp(s["panels"][l]), S()) == 0
    s["words"] = [torch.zeros(P + 1, 5, dtype=torch.int32, device=DEV) for _ in range(n)]
    return s


def chain_call(s, **kw):
    a = dict(s, **kw)
    null = lambda key, mk: None if a[key] is None else mk(a[key])
    return L().d3ga_mlp_chain_fwd(a["P"], a["K0"], vp(a["X"]), a["L"], null("Ks", lambda v: c_arr(i32, v)), null("Ns", lambda v: c_arr(i32, v)),
                                  null("panels", ptr_arr), null("biases", ptr_arr), null("slopes", lambda v: c_arr(ctypes.c_float, v)),
                                  null("outs", ptr_arr), null("signs", ptr_arr), null("masks", ptr_arr),
                                  null("mask_slopes", lambda v: c_arr(ctypes.c_float, v)), S())


def edited(lst, l, v):
    out = list(lst)
    out[l] = v
    return out


def test_chain_fwd_refusals():
    """Every D3GA_E_* branch of d3ga_mlp_chain_fwd, each leaving the outputs, the sign words AND the panels (their bias tails
    included: the bias launch used to run before the masks-with-forward-arithmetic refusal) as they were."""
    s = chain_refusal_scene()
    fz = Frozen(*s["panels"], *s["outs"], *s["signs"])
    none9, ones9 = [None] * 9, [1.0] * 9
    bwd_ok = dict(biases=None, slopes=ones9, signs=none9)                   # what a call with masks needs
    cases = [
        ("P < 0", dict(P=-1), E_SIZE), ("L = 0", dict(L=0), E_SIZE), ("L = 9", dict(L=9), E_SIZE), ("K0 = 0", dict(K0=0), E_SIZE),
        ("K0 = 129", dict(K0=129, Ks=edited(s["Ks"], 0, 129)), E_SIZE),
        ("Ks[0] != K0", dict(Ks=edited(s["Ks"], 0, 13)), E_SIZE), ("Ks[2] != Ns[1]", dict(Ks=edited(s["Ks"], 2, 127)), E_SIZE),
        ("Ns[2] = 0", dict(Ns=edited(s["Ns"], 2, 0)), E_SIZE), ("Ns[2] = 129", dict(Ns=edited(s["Ns"], 2, 129)), E_SIZE),
        ("X NULL", dict(X=None), E_NULL), ("Ks NULL", dict(Ks=None), E_NULL), ("Ns NULL", dict(Ns=None), E_NULL),
        ("panels NULL", dict(panels=None), E_NULL), ("slopes NULL", dict(slopes=None), E_NULL), ("outs NULL", dict(outs=None), E_NULL),
        ("signs NULL", dict(signs=None), E_NULL),
        ("panels[1] NULL", dict(panels=edited(s["panels"], 1, None)), E_NULL), ("outs[2] NULL", dict(outs=edited(s["outs"], 2, None)), E_NULL),
        ("panels[1] + 4", dict(panels=edited(s["panels"], 1, s["panels"][1].ptr() + 4)), E_CONFIG),
        ("outs[0] + 4", dict(outs=edited(s["outs"], 0, s["outs"][0].ptr() + 4)), E_CONFIG),
        ("outs[2] + 8", dict(outs=edited(s["outs"], 2, s["outs"][2].ptr() + 8)), E_CONFIG),
        ("masks[0] + 4 (four words a row)", dict(bwd_ok, masks=edited(none9, 0, s["words"][0].data_ptr() + 4)), E_CONFIG),
        ("L = 1", dict(L=1), E_CONFIG), ("a hidden layer 64 wide", dict(Ns=edited(s["Ns"], 0, 64), Ks=edited(s["Ks"], 1, 64)), E_CONFIG),
        ("masks with a bias", dict(bwd_ok, biases=s["biases"], masks=s["words"]), E_CONFIG),
        ("masks with a bias on one layer", dict(bwd_ok, biases=edited(none9, 2, s["biases"][2]), masks=edited(none9, 1, s["words"][1])), E_CONFIG),
        ("masks with an activation", dict(bwd_ok, slopes=edited(ones9, 1, 0.1), masks=s["words"]), E_CONFIG),
        ("masks with a sign output", dict(bwd_ok, signs=edited(none9, 0, s["signs"][0]), masks=s["words"]), E_CONFIG),
    ]
    for tag, kw, want in cases:
        assert chain_call(s, **kw) == want, tag
        fz.same(tag)
    assert chain_call(s, P=0) == 0
    assert chain_call(s, P=0, X=None, panels=None, outs=None) == 0
    fz.same("P = 0")
    # a mask array whose entries are all NULL refuses nothing, whatever the arithmetic; and the base call is a valid one
    assert chain_call(s, masks=none9) == 0
    assert chain_call(s) == 0
    assert chain_call(s, **dict(bwd_ok, masks=s["words"], mask_slopes=ones9)) == 0
    torch.cuda.synchronize()
