"""Host-side checks of the barycentric attribute interpolation (d3ga_amd/bary_interp.py): the binding's plan against brute force
on CPU tensors, the refusal table of d3ga_bary_interp_{fwd,bwd} with pointers that are never read, and the float64 restatement
of tests/bary_ref.py against the fixture recorded from the reference's own forwards (tools/gen_golden.py G14).  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import bary_ref
from d3ga_amd import D3GAError
from d3ga_amd.bary_interp import BaryBinding


def _check_plan(b, final, n_rows):
    assert b.rows.dtype == torch.int32 and b.rows.is_contiguous() and torch.equal(b.rows.long(), final)
    assert (b.n_rows, b.K, b.P) == (n_rows, final.shape[1], final.shape[0])
    assert b.vert_start.dtype == torch.int32 and b.vert_items.dtype == torch.int32
    assert b.vert_start.shape == (n_rows + 1,) and b.vert_items.shape == (final.numel(),)
    lists = bary_ref.brute_force_lists(final, n_rows)
    start, items = b.vert_start.tolist(), b.vert_items.tolist()
    assert start[0] == 0 and start[-1] == final.numel()
    for v in range(n_rows):
        assert items[start[v]:start[v + 1]] == lists[v], v          # fixed order: ascending item K i + k
    return lists


def test_binding_cage_form_against_brute_force():
    g = torch.Generator().manual_seed(3)
    cells = torch.randint(0, 20, (37, 4), generator=g)
    cell_id = torch.randint(0, 37, (101,), generator=g)
    b = BaryBinding(cells=cells, cell_id=cell_id, n_rows=23)
    lists = _check_plan(b, cells[cell_id], 23)
    assert any(len(l) == 0 for l in lists[20:])                       # rows 20..22 are read by nobody: empty lists
    # int32 index tensors give the same plan
    b32 = BaryBinding(cells=cells.int(), cell_id=cell_id.int(), n_rows=23)
    assert torch.equal(b32.rows, b.rows) and torch.equal(b32.vert_items, b.vert_items)


def test_binding_table_form_and_empty_binding():
    g = torch.Generator().manual_seed(4)
    rows = torch.randint(0, 9, (64, 3), generator=g)
    rows[rows == 5] = 6                                               # row 5 has an empty list between two used ones
    lists = _check_plan(BaryBinding(rows, n_rows=9), rows, 9)
    assert lists[5] == [] and lists[4] and lists[6]
    empty = BaryBinding(torch.zeros((0, 4), dtype=torch.int64), n_rows=7)
    assert empty.P == 0 and empty.K == 4 and empty.vert_start.tolist() == [0] * 8 and empty.vert_items.numel() == 0


def test_binding_many_to_one_vertex_map_lists_follow_the_final_rows():
    g = torch.Generator().manual_seed(5)
    cells = torch.randint(0, 27, (48, 4), generator=g)
    cell_id = torch.randint(0, 48, (60,), generator=g)
    vmap = torch.randint(0, 10, (27,), generator=g)
    vmap[vmap == 7] = 2                                               # 27 cage vertices onto 10 of 11 body vertices, 7 unused
    b = BaryBinding(cells=cells, cell_id=cell_id, vertex_map=vmap, n_rows=11)
    final = vmap[cells[cell_id]]
    lists = _check_plan(b, final, 11)
    assert lists[7] == [] and lists[10] == [] and max(map(len, lists)) > 16
    # a table seen through a map
    rows = torch.randint(0, 27, (33, 3), generator=g)
    _check_plan(BaryBinding(rows, vertex_map=vmap, n_rows=11), vmap[rows], 11)


def test_binding_refuses_bad_ids_and_shapes():
    cells = torch.tensor([[0, 1, 2, 3], [1, 2, 3, 4]])
    ok_id = torch.tensor([0, 1, 1])
    BaryBinding(cells=cells, cell_id=ok_id, n_rows=5)
    with pytest.raises(D3GAError, match="outside"):
        BaryBinding(cells=cells, cell_id=ok_id, n_rows=4)                                   # vertex 4 >= n_rows
    with pytest.raises(D3GAError, match="cell_id"):
        BaryBinding(cells=cells, cell_id=torch.tensor([0, 2]), n_rows=5)                    # cell 2 of 2
    with pytest.raises(D3GAError, match="cell_id"):
        BaryBinding(cells=cells, cell_id=torch.tensor([-1, 0]), n_rows=5)
    with pytest.raises(D3GAError, match="outside"):
        BaryBinding(torch.tensor([[0, 1, -1]]), n_rows=5)
    with pytest.raises(D3GAError, match="outside"):
        BaryBinding(torch.tensor([[0, 1, 5]]), n_rows=5)
    with pytest.raises(D3GAError, match="outside"):                                         # beyond the map's length
        BaryBinding(cells=cells, cell_id=ok_id, vertex_map=torch.tensor([0, 1, 2, 3]), n_rows=5)
    with pytest.raises(D3GAError, match="outside"):                                         # the map itself points too far
        BaryBinding(cells=cells, cell_id=ok_id, vertex_map=torch.tensor([0, 1, 2, 3, 9]), n_rows=5)
    with pytest.raises(D3GAError, match="K = 2"):
        BaryBinding(torch.tensor([[0, 1]]), n_rows=5)
    with pytest.raises(D3GAError, match="either"):
        BaryBinding(torch.tensor([[0, 1, 2]]), cells=cells, cell_id=ok_id, n_rows=5)
    with pytest.raises(D3GAError, match="either"):
        BaryBinding(cells=cells, n_rows=5)
    with pytest.raises(D3GAError, match="int32 or int64"):
        BaryBinding(torch.tensor([[0.0, 1.0, 2.0]]), n_rows=5)


def test_binding_is_cached_on_its_index_tensors():
    cells = torch.tensor([[0, 1, 2, 3], [1, 2, 3, 4]])
    cell_id = torch.tensor([0, 1, 1])
    a = BaryBinding(cells=cells, cell_id=cell_id, n_rows=5)
    assert BaryBinding(cells=cells, cell_id=cell_id, n_rows=5) is a
    assert BaryBinding(cells=cells, cell_id=cell_id, n_rows=6) is not a                     # another attribute length
    vmap = torch.arange(5)
    m = BaryBinding(cells=cells, cell_id=cell_id, vertex_map=vmap, n_rows=5)
    assert m is not a and BaryBinding(cells=cells, cell_id=cell_id, vertex_map=vmap, n_rows=5) is m
    cell_id[0] = 1                                                                          # an in-place edit is a new binding
    c = BaryBinding(cells=cells, cell_id=cell_id, n_rows=5)
    assert c is not a and c.rows[0].tolist() == [1, 2, 3, 4]


def test_bary_interp_entry_points_refuse_bad_arguments_no_gpu_needed():
    """The status table of d3ga_bary_interp_{fwd,bwd} (include/d3ga.h D2b) for what is decided before any HIP call: every
    pointer below is a made-up non-NULL address that is never read."""
    import d3ga_amd
    L = d3ga_amd.lib()
    OK, E_NULL, E_SIZE, E_CONFIG = 0, -1, -2, -3
    p, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)

    def fwd(P=4, K=4, C=3, attr=p, rows=p, barys=p, delta=None, out=p):
        return L.d3ga_bary_interp_fwd(P, K, C, attr, rows, barys, delta, out, None)

    def bwd(P=4, V=5, K=4, C=3, attr=p, rows=p, barys=p, delta=None, g_out=p, vert_start=p, vert_items=p, g_attr=p, g_barys=p):
        return L.d3ga_bary_interp_bwd(P, V, K, C, attr, rows, barys, delta, g_out, vert_start, vert_items, g_attr, g_barys, None)
    # sizes: negative, K outside {3, 4}, C outside 1..8, K P beyond int32 -- decided first, whatever the pointers
    for kw in (dict(P=-1), dict(K=2), dict(K=5), dict(K=0), dict(C=0), dict(C=9), dict(C=-1), dict(P=2**30, K=4), dict(P=2**30, K=3)):
        assert fwd(**kw) == E_SIZE, kw
        assert bwd(**kw) == E_SIZE, kw
        assert fwd(attr=None, **kw) == E_SIZE and bwd(g_out=None, **kw) == E_SIZE, kw
    assert bwd(V=-1) == E_SIZE
    # P == 0: nothing to do, no pointer is looked at
    assert fwd(P=0, attr=None, rows=None, barys=None, out=None) == OK
    assert bwd(P=0, attr=None, rows=None, barys=None, g_out=None, vert_start=None, vert_items=None, g_attr=None, g_barys=None) == OK
    assert bwd(P=0, V=0, attr=None, rows=None, barys=None, g_out=None, vert_start=None, vert_items=None, g_barys=None) == OK
    # a required pointer
    for name in ("attr", "rows", "barys", "out"):
        assert fwd(**{name: None}) == E_NULL, name
        assert fwd(K=3, **{name: None}) == E_NULL, name
    for name in ("attr", "rows", "barys", "g_out"):
        assert bwd(**{name: None}) == E_NULL, name
        assert bwd(g_attr=None, vert_start=None, vert_items=None, **{name: None}) == E_NULL, name
    # g_attr is a gather: it needs both lists (there is no float-atomic fallback)
    assert bwd(vert_start=None) == E_NULL and bwd(vert_items=None) == E_NULL and bwd(K=3, vert_start=None, vert_items=None) == E_NULL
    # K == 4 moves 16 bytes per Gaussian
    for name in ("rows", "barys", "delta"):
        assert fwd(**{name: odd}) == E_CONFIG, name
        assert bwd(**{name: odd}) == E_CONFIG, name
    assert bwd(g_barys=odd) == E_CONFIG


def test_op_refuses_cpu_tensors():
    """There is no CPU fallback: the plan builds on the CPU, the op does not run there."""
    from d3ga_amd.bary_interp import bary_interp, mesh_means
    rows = torch.tensor([[0, 1, 2], [1, 2, 3]])
    with pytest.raises(D3GAError, match="GPU only"):
        bary_interp(torch.zeros(4, 3), BaryBinding(rows, n_rows=4), torch.zeros(2, 3))
    with pytest.raises(D3GAError, match="GPU only"):
        mesh_means(torch.zeros(4, 3), rows, torch.zeros(2, 3))
    with pytest.raises(D3GAError, match="BaryBinding"):
        bary_interp(torch.zeros(4, 3), rows, torch.zeros(2, 3))


def test_abi_version_is_unchanged():
    import d3ga_amd
    from d3ga_amd import _lib
    assert _lib.ABI_VERSION == 112 and d3ga_amd.lib().d3ga_version() == 112
    assert {"d3ga_bary_interp_fwd", "d3ga_bary_interp_bwd"} <= set(_lib.EXPORTS)


@pytest.mark.parametrize("name", ["shadow", "canonical", "mesh", "mesh_canonical"])
def test_float64_restatement_matches_the_reference_fixture(golden, name):
    """Pins the oracle of the GPU tests to the reference: its float32 results lie within ONE bar of the float64 restatement
    (the bound of any float32 summation order)."""
    c = bary_ref.golden_cases(golden("interp_cases.npz"))[name]
    rows = bary_ref.final_rows(**c["bind"])
    K, C = rows.shape[1], 1 if c["attr"].dim() == 1 else c["attr"].shape[1]
    assert c["out"].dtype == torch.float32 and c["out"].shape == (rows.shape[0], C)
    ref = bary_ref.interp_ref(c["attr"], rows, c["barys"], c["delta"], c["up"])
    bar = bary_ref.bars(ref, K, C)
    bary_ref.assert_within(f"{name} out", c["out"], ref["out"], bar["out"])
    if c["up"] is not None:
        bary_ref.assert_within(f"{name} g_attr", c["g_attr"], ref["g_attr"], bar["g_attr"])
        bary_ref.assert_within(f"{name} g_barys", c["g_barys"], ref["g_barys"], bar["g_barys"])
        assert float(ref["g_attr"].abs().max()) > 0 and float(ref["g_barys"].abs().max()) > 0
    if name == "shadow":                                   # the fixture's shape: long lists behind the map, one unused body vertex
        assert ref["L"].max() > 16 and ref["L"][7] == 0 and c["attr"].shape == (11,)
