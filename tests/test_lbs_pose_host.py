"""Host side of the D0 pose gradients (no GPU): sparse_skin_weights, the by-joint plan of the pose backward, its refusals, and the
C ABI struct (include/d3ga.h: d3ga_lbs_pose_grad)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from d3ga_amd import _lib
from d3ga_amd.cage_deform import lbs_pose_plan, sparse_skin_weights
from oracle import deform as od

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dense_table(V, J, max_nz, seed):
    g = torch.Generator().manual_seed(seed)
    W = torch.zeros(V, J, dtype=torch.float64)
    for v in range(V):
        n = int(torch.randint(1, max_nz + 1, (1,), generator=g))
        cols = torch.randperm(J, generator=g)[:n]
        W[v, cols] = torch.rand(n, generator=g, dtype=torch.float64) + 0.05
    return W / W.sum(1, keepdim=True)


@pytest.mark.parametrize("V,J,max_nz,K", [(200, 55, 4, None), (50, 6, 6, None), (30, 10, 3, 8), (7, 3, 3, 5), (1, 1, 1, None)])
def test_sparse_skin_weights_equal_the_dense_product(V, J, max_nz, K):
    """The K-sparse form gives the dense product W A: the reference's T = skin_weights . A (lib/smplman.py:157) on the rows
    nn_ids, here in float64 on the CPU through the oracle's K-sparse skinning."""
    W = _dense_table(V + 5, J, max_nz, seed=V + J)
    rows = torch.arange(V + 5).flip(0)[:V]
    idx, w = sparse_skin_weights(W, rows=rows, K=K)
    kmax = int((W[rows] != 0).sum(1).max())
    assert idx.dtype == torch.int32 and idx.shape == (V, K if K is not None else kmax) and w.shape == idx.shape
    assert int(idx.min()) >= 0 and int(idx.max()) < J
    g = torch.Generator().manual_seed(3)
    A = torch.randn(J, 4, 4, generator=g, dtype=torch.float64)
    tmpl = torch.randn(V, 3, generator=g, dtype=torch.float64)
    got = od.lbs_cage(tmpl, None, A, idx.long(), w)
    T = (W[rows] @ A.reshape(J, 16)).reshape(V, 4, 4)
    want = (T[:, :3, :3] @ tmpl[:, :, None])[:, :, 0] + T[:, :3, 3]
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    # every non-zero weight kept exactly, once, with its joint; the padding carries weight 0
    for v in range(V):
        kept = {int(j): float(x) for j, x in zip(idx[v], w[v]) if x != 0}
        ref = {int(j): float(W[rows[v], j]) for j in torch.nonzero(W[rows[v]]).reshape(-1)}
        assert kept == ref


def test_sparse_skin_weights_refusals():
    W = _dense_table(10, 8, 4, seed=1)
    kmax = int((W != 0).sum(1).max())
    with pytest.raises(ValueError, match="drops weights"):
        sparse_skin_weights(W, K=kmax - 1)
    with pytest.raises(ValueError, match=r"\(V,J\)"):
        sparse_skin_weights(W[0])


@pytest.mark.parametrize("V,K,J,seed", [(1, 1, 1, 0), (24000 // 8, 4, 55, 1), (100, 24, 5, 2), (700, 8, 160, 3), (40, 3, 300, 4)])
def test_pose_plan_invariants(V, K, J, seed):
    """entries are a permutation of 0..V*K-1 sorted by joint (stable); chunks tile each joint's run with at most 256 entries and
    never straddle a joint; chunk_ptr gives each joint its chunks, a joint without entries none.  SMPL-X-like skew: joint 0
    carries a large share of the entries."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, J, (V, K), generator=g)
    idx[: V // 2, 0] = 0
    plan = lbs_pose_plan(idx.to(torch.int32), J)
    flat = idx.reshape(-1)
    ent = plan["entries"].long()
    assert plan["n_entries"] == V * K and plan["J"] == J and int(plan["counter"][0]) == 0
    assert torch.equal(torch.sort(ent)[0], torch.arange(V * K))
    js = flat[ent]
    assert bool((js[1:] >= js[:-1]).all())
    same = js[1:] == js[:-1]
    assert bool((ent[1:][same] > ent[:-1][same]).all())                      # stable: entries of a joint in flat order
    rng, ptr = plan["chunk_range"].long(), plan["chunk_ptr"].long()
    assert rng.shape == (plan["n_chunks"], 2) and ptr.shape == (J + 1,) and int(ptr[-1]) == plan["n_chunks"]
    counts = torch.bincount(flat, minlength=J)
    pos = 0
    for j in range(J):
        cs = rng[int(ptr[j]):int(ptr[j + 1])]
        assert cs.shape[0] == (int(counts[j]) + 255) // 256
        for b, e in cs.tolist():
            assert b == pos and 0 < e - b <= 256
            assert bool((js[b:e] == j).all())
            pos = e
    assert pos == V * K
    # cached by the storage of skin_idx and J
    i32 = idx.to(torch.int32)
    assert lbs_pose_plan(i32, J) is lbs_pose_plan(i32, J)
    assert lbs_pose_plan(i32, J + 1) is not lbs_pose_plan(i32, J)


def test_pose_plan_refuses_out_of_range_indices():
    idx = torch.zeros(5, 3, dtype=torch.int32)
    idx[3, 2] = 7
    with pytest.raises(ValueError, match=r"skin_idx\[3, 2\] = 7 is outside \[0, 7\)"):
        lbs_pose_plan(idx, 7)
    idx[3, 2] = -1
    with pytest.raises(ValueError, match=r"skin_idx\[3, 2\] = -1"):
        lbs_pose_plan(idx, 7)
    with pytest.raises(ValueError, match="at least one joint"):
        lbs_pose_plan(torch.zeros(2, 2, dtype=torch.int32), 0)


def _header_struct(hdr, name):
    """(field names, sizeof) of `typedef struct name {...} name;` as the C compiler lays it out: int32 4 bytes, int64 and
    pointers 8, each aligned to its size, the total to 8."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    names, off = [], 0
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        first, *more = decl.split(",")                       # `type a, *b`: the `*` belongs to each declarator
        ctype = first[:re.search(r"\*?\s*\w+$", first).start()].strip()
        for item in [first[len(ctype):]] + more:
            size = 8 if ("*" in item or "int64_t" in ctype) else 4
            assert size == 8 or "int32_t" in ctype, decl
            off = (off + size - 1) // size * size + size
            names.append(re.search(r"(\w+)$", item.strip()).group(1))
    return names, (off + 7) // 8 * 8


def test_pose_struct_matches_the_header():
    """struct d3ga_lbs_pose_grad: the ctypes mirror has the header's fields in order, 8-byte pointers after two int32 and an int64;
    the descriptor structs of d3ga_cage_deform_{fwd,bwd} are held to the same."""
    with open(os.path.join(ROOT, "include", "d3ga.h")) as f:
        hdr = f.read()
    body = re.search(r"typedef struct d3ga_lbs_pose_grad \{(.*?)\} d3ga_lbs_pose_grad;", hdr, re.S).group(1)
    names = re.findall(r"\*?(\w+);", body)
    assert names == [n for n, _ in _lib.LbsPoseGrad._fields_]
    assert ctypes.sizeof(_lib.LbsPoseGrad) == 16 + 10 * 8
    assert _header_struct(hdr, "d3ga_lbs_pose_grad") == (names, 16 + 10 * 8)
    for cname, mirror, size in (("d3ga_cage_deform_in", _lib.CageDeformIn, 16 + 8 * 8), ("d3ga_cage_deform_grads", _lib.CageDeformGrads, 6 * 8),
                                ("d3ga_cage_deform_route", _lib.CageDeformRoute, 8 + 6 * 8), ("d3ga_cage_deform_skin", _lib.CageDeformSkin, 8 + 6 * 8)):
        names, sizeof = _header_struct(hdr, cname)
        assert names == [n for n, _ in mirror._fields_], cname
        assert ctypes.sizeof(mirror) == sizeof == size, cname
    for key in ("CORNERS", "MERGE"):
        assert int(re.search(r"#define\s+D3GA_DEFORM_ROUTE_%s\s+(\d+)" % key, hdr).group(1)) == getattr(_lib, "DEFORM_ROUTE_" + key)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("d3ga_lbs_pose_scratch_bytes", "d3ga_lbs_cage_bwd", "d3ga_cage_deform_fwd", "d3ga_cage_deform_bwd"):
        assert name in _lib.EXPORTS and re.search(r"int " + name + r"\(", hdr)
    for name in ("d3ga_lbs_cage_bwd_pose", "d3ga_cage_deform_fwd_ex", "d3ga_cage_deform_bwd_ex", "d3ga_cage_deform_bwd_merged",
                 "d3ga_cage_deform_bwd_merged_lbs", "d3ga_cage_deform_bwd_merged_lbs_pose"):
        assert name not in _lib.EXPORTS and not re.search(r"\b" + name + r"\b", code)
    assert np.int32(_lib.ABI_VERSION) == 112
