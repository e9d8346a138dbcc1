"""Float64 side of tests/test_gpu_mlp_paths.py, written from the formulas of include/d3ga.h ("Field networks"): the dense
layer with its output slope, the sign words, the mask multiply, the weight and bias gradient, a trunk forward and the backward's
input-gradient chain as the header defines it, plus the tables of the test (which template instantiation of the launcher a shape
reaches, the pairwise covers).  CPU only; every tensor in, float64 out.  A weight matrix here is always `Wkn` (K, N):
Wkn[k][n] = the weight of input k for output n, the header's weight(k, n)."""
import itertools

import torch


def dense(x, Wkn, bias=None, out_slope=1.0):
    """Y = act_out(X . W + bias), act_out(y) = y > 0 ? y : out_slope y."""
    y = x.double() @ Wkn.double()
    if bias is not None:
        y = y + bias.double()
    return torch.where(y > 0, y, out_slope * y)


def n_words(N):
    return (N + 31) // 32


def pack_signs(pos):
    """bool (P, N) -> int32 (P, ceil(N/32)) holding the uint32 words: bit (n & 31) of word [r][n >> 5] = pos[r][n]."""
    P, N = pos.shape
    nw = n_words(N)
    bits = torch.zeros(P, nw * 32, dtype=torch.int64)
    bits[:, :N] = pos.to(torch.int64)
    w = (bits.view(P, nw, 32) << torch.arange(32, dtype=torch.int64)).sum(-1)          # 0 .. 2^32 - 1
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def unpack_signs(words, N):
    """int32 words (P, ceil(N/32)) -> bool (P, N)."""
    w = words.cpu().to(torch.int64) & 0xFFFFFFFF
    bits = (w[:, :, None] >> torch.arange(32, dtype=torch.int64)) & 1
    return bits.reshape(w.shape[0], -1)[:, :N].bool()


def mask_factor(bits, mask_slope, dtype=torch.float64):
    """bit ? 1 : mask_slope per element."""
    return torch.where(bits, torch.ones((), dtype=dtype), torch.full((), mask_slope, dtype=dtype))


def wgrad(dpre, x):
    """dW (N, K) = dPre^T . X and db (N) = column sums of dPre."""
    return dpre.double().T @ x.double(), dpre.double().sum(0)


def trunk_forward(x, layers, slopes):
    """h_{l+1} = act_l(h_l W_l + b_l); layers = [(Wkn, bias or None)] -> the list of every layer's output."""
    outs, h = [], x.double()
    for (W, b), s in zip(layers, slopes):
        h = dense(h, W, b, s)
        outs.append(h)
    return outs


def chain_backward(g, mats, masks, mask_slopes):
    """The backward's input-gradient chain as one call of d3ga_mlp_chain_fwd sees it: X = g, layer l multiplies by mats[l]
    (Wkn of the CALL: the transposed weights of a model layer) and then by (bit ? 1 : mask_slopes[l]) where masks[l] (bool,
    shape of the output) is not None -> every layer's output."""
    outs, h = [], g.double()
    for W, m, s in zip(mats, masks, mask_slopes):
        h = h @ W.double()
        if m is not None:
            h = h * mask_factor(m, s)
        outs.append(h)
    return outs


# ------------------------------------------------------------------------------------------------------------------------
# which instantiations linear_kernel<NB, VEC, EMASK, RAGGED> a call of d3ga_mlp_linear launches (its launcher, restated):
# rows [0, P - P % 32) without bounds checks when n_out is a multiple of 32, the rest (or everything) bounds-checked
# ------------------------------------------------------------------------------------------------------------------------
def linear_instances(P, K, n_out, mask):
    NB, vec = n_words(n_out), K % 4 == 0
    p_full = P - P % 32 if n_out % 32 == 0 else 0
    inst = []
    if p_full > 0:
        inst.append((NB, vec, bool(mask), False))
    if P - p_full > 0:
        inst.append((NB, vec, bool(mask), True))
    return inst


def inst_name(i):
    return f"NB{i[0]}{'v' if i[1] else 's'}{'m' if i[2] else '-'}{'R' if i[3] else 'F'}"


ALL_LINEAR_INSTANCES = set(itertools.product((1, 2, 3, 4), (False, True), (False, True), (False, True)))

LIN_NOUT = (32, 64, 96, 128, 1, 11, 33, 65, 97, 127)
LIN_K = (1, 3, 4, 11, 16, 17, 48, 127, 128)
LIN_P = (1, 31, 32, 33, 511, 512, 513, 545)


def _mix(i, j, c):
    """A fixed 32-bit hash of the cell (i, j): deals the remaining factors of a table.  The constants c below are the first for
    which the table is a pairwise cover (the test asserts that it is)."""
    h = ((i * 31 + j * 17 + c) * 2654435761) & 0xFFFFFFFF
    h ^= h >> 15
    h = (h * 2246822519) & 0xFFFFFFFF
    return h ^ (h >> 13)


def linear_table():
    """One row per (n_out, K): P, mask, sign, bias and slope are dealt so that every pair of values of two factors meets in some
    row (pairs_missing() == [] is asserted by the test) -> dicts with the instantiations each row reaches."""
    rows = []
    for i, n_out in enumerate(LIN_NOUT):
        for j, K in enumerate(LIN_K):
            h = _mix(i, j, 2)
            r = dict(n_out=n_out, K=K, P=LIN_P[(i + j) % 8], mask=bool(h & 1), sign=bool(h & 2), bias=bool(h & 4),
                     slope=(1.0, 0.1)[(h >> 3) & 1])
            r["inst"] = linear_instances(r["P"], K, n_out, r["mask"])
            r["id"] = f"P{r['P']}_K{K}_N{n_out}_{'m' if r['mask'] else '-'}{'s' if r['sign'] else '-'}{'b' if r['bias'] else '-'}" \
                      f"_a{r['slope']}_" + "+".join(inst_name(x) for x in r["inst"])
            rows.append(r)
    return rows


CHAIN_L = (2, 3, 4, 5, 6, 7, 8)
CHAIN_K0 = (1, 3, 4, 5, 32, 33, 64, 65, 96, 97, 128)
CHAIN_LAST = (1, 3, 4, 32, 33, 64, 96, 100, 128)
CHAIN_BIAS = ("all", "absent", "some")          # every layer | biases == NULL | biases[l] == NULL on every other layer
CHAIN_SLOPES = ((0.1, 1.0), (0.01, 0.2), (1.0, 1.0))      # (hidden layers, last layer)
CHAIN_ROWS = (256 * 2 + 37, 256 * 5 + 1, 256 * 3, 1)


def chain_table():
    """One row per (K0, last width); L, bias mode, slopes, sign output and the 4-byte offset of X dealt for a pairwise cover."""
    rows = []
    for i, K0 in enumerate(CHAIN_K0):
        for j, last in enumerate(CHAIN_LAST):
            h = _mix(i, j, 6)
            r = dict(K0=K0, last=last, L=CHAIN_L[(i + j) % 7], bias=CHAIN_BIAS[(h >> 4) % 3], slopes=CHAIN_SLOPES[(h >> 8) % 3],
                     signs=bool(h & 1), xoff=bool(h & 2))
            r["nch0"], r["ntl"] = (K0 + 31) // 32, n_words(last)
            r["id"] = f"L{r['L']}_K{K0}_N{last}_b{r['bias']}_s{r['slopes'][0]}-{r['slopes'][1]}_{'sg' if r['signs'] else '--'}" \
                      f"_{'x4' if r['xoff'] else 'x16'}_nch{r['nch0']}_NTL{r['ntl']}"
            rows.append(r)
    return rows


def pairs_missing(rows, factors):
    """The pairs of values (of two different factors: name -> all its values) that no row of the table has together."""
    missing = []
    for (fa, va), (fb, vb) in itertools.combinations(factors.items(), 2):
        have = {(r[fa], r[fb]) for r in rows}
        missing += [(fa, a, fb, b) for a in va for b in vb if (a, b) not in have]
    return missing
