"""Quadric edge-collapse decimation on the GPU (d3ga_amd/cage_author.py::decimate, csrc/decimate.hip): the kernels against the g++
build of csrc/decimate_math.h (tests/decimate_ref.py) -- bit for bit in faces, vertices, rounds and status, since a last bit of a
cost can change which edge wins -- on the meshes of the host test, on 5 668 faces (23 scan blocks, V and E no multiples of 256),
on 69 720 faces (the block totals take a second pass) and on the edge cases.  The g++ build itself is held to the numpy oracle
and to first principles in tests/test_decimate_host.py."""
import numpy as np
import pytest
import torch

import cage_author_ref as ca
import decimate_ref as dr
import template_bind_ref as tr

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = {name: (v, f, t, dr.MAX_ROUNDS) for gen in (dr.host_cases, dr.large_cases) for name, v, f, t in gen()}
CASES.update({name: (v, f, t, m) for name, v, f, t, m in dr.small_cases()})
_CACHE = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def shared(key, make):
    """references are computed once and never written to"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def run(v, f, target, max_rounds=dr.MAX_ROUNDS):
    from d3ga_amd import decimate
    out = decimate(dev(v), dev(f), tris_target=target, max_rounds=max_rounds)
    assert out.vertices.dtype == torch.float32 and out.faces.dtype == torch.int32 and out.vertices.is_cuda and out.status.shape == (1,)
    return host(out.vertices), host(out.faces), out.rounds, int(out.status.item())


@pytest.mark.parametrize("name", list(CASES))
def test_kernels_equal_the_host_build_bit_for_bit(name):
    v, f, target, max_rounds = CASES[name]
    if "fills" in name:
        assert len(f) > 65536
    want = shared(name, lambda: dr.host_decimate(v, f, target, max_rounds))
    dr.same_result(run(v, f, target, max_rounds), want)


def test_check_raises_when_stuck():
    from d3ga_amd import decimate
    v, f = tr.tetrahedron()
    out = decimate(dev(v), dev(f), tris_target=2)
    assert out.rounds == 1 and torch.equal(out.faces, dev(f))
    with pytest.raises(ValueError, match="stopped at 4 faces after 1 rounds, the target was 2"):
        out.check()
    vertices, faces = decimate(dev(v), dev(f), tris_target=4).check()        # nothing to do: the identity, and it unpacks
    assert torch.equal(faces, dev(f)) and torch.equal(vertices, dev(v).float())


def test_a_second_call_and_a_permuted_input():
    name = "capsule figure r=8 -> 400"
    v, f, target, _ = CASES[name]
    first = run(v, f, target)
    dr.same_result(run(v, f, target), first)
    pv, pf = tr.shuffled(v, f, 3)
    dr.same_result(run(pv, pf, target), shared((name, "permuted"), lambda: dr.host_decimate(pv, pf, target)))
    dr.same_result(run(v.astype(np.float32), f.astype(np.int64), target), dr.host_decimate(v.astype(np.float32), f, target))     # the other dtypes


def test_a_non_manifold_edge_is_refused():
    from d3ga_amd import decimate
    v, f = tr.tetrahedron()
    v, f = np.concatenate([v, [[2.0, 2, 2]]]), np.concatenate([f, [[0, 1, 4]]]).astype(np.int32)
    with pytest.raises(ValueError, match="more than 2 faces"):
        decimate(dev(v), dev(f), tris_target=2)


def test_cage_processor_end_to_end_with_decimation():
    """`cage_processor(..., decimation="quadric")` against the g++ build of the decimation and of the component filter, fed with the
    device's own Taubin-filtered surface (the smoothers meet their g++ build to 2^-23 only -- acos is a library call -- and have
    tests of their own): identical bits.  Shapes and dtypes as the reference returns them; the count, closedness, Euler
    characteristic and orientation from first principles."""
    from d3ga_amd import cage_processor, create_cage, smooth_cage, smooth_taubin
    v, f = shared(("mesh", "figure"), ca.capsule_figure)
    radius = 12
    cv, cf = create_cage(dev(v), dev(f), radius, 0.01)
    sv, sf = smooth_cage(cv, cf)
    tv = smooth_taubin(sv, sf, iterations=10).check().vertices
    target = cf.shape[0] // 3
    want_v, want_f = dr.host_tail(host(tv), host(sf), target)
    out_v, out_f = cage_processor(dev(v), dev(f), cage_tris_target=target, radius=radius, decimation="quadric")
    assert out_v.dtype == torch.float32 and out_f.dtype == torch.int64 and out_v.is_cuda and out_f.is_cuda
    assert out_v.shape == (1, len(want_v), 3) and out_f.shape == (1, len(want_f), 3)
    assert ca.same_bits(host(out_v[0]), want_v) and np.array_equal(host(out_f[0]), want_f)
    got_v, got_f = host(out_v[0]), host(out_f[0])
    assert len(got_f) in (target, target - 1) and len(got_f) >= 70 and dr.parts(got_f) == 1
    assert ca.edge_census(got_f)[:2] == (True, True) and dr.euler(got_f) == 2 and ca.signed_volume(got_v, got_f) > 0
    with pytest.raises(NotImplementedError, match="quadric decimation is not built yet"):
        cage_processor(dev(v), dev(f), cage_tris_target=target, radius=radius)


def test_simplify_is_the_chain_called_by_hand():
    from d3ga_amd import decimate, keep_components, simplify, smooth_taubin
    v, f = CASES["capsule figure r=16 -> 1232"][:2]
    target = 1500
    got_v, got_f = simplify(dev(v), dev(f), tris_target=target, decimation="quadric")
    tv = smooth_taubin(dev(v), dev(f), iterations=10).check().vertices
    dv, df = decimate(tv, dev(f), tris_target=target).check()
    want_v, want_f = keep_components(dv, df, min_faces=70)
    assert torch.equal(got_v, want_v) and torch.equal(got_f, want_f) and got_f.shape[0] in (target, target - 1)
    plain_v, plain_f = simplify(dev(v), dev(f), tris_target=0, decimation="quadric")          # no target: nothing is decimated
    assert plain_f.shape[0] == len(f)
