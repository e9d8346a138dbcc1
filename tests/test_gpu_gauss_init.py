"""Gaussian initialisation on the GPU (d3ga_amd/gauss_init.py, csrc/gauss_init.hip) against the g++ build of csrc/gauss_init_math.h
(tests/gauss_init_ref.py; itself held to the numpy oracle and to the reference's own functions by tests/test_gauss_init_host.py):
the kernels give its bits for every output, between guard bands, for face counts on both sides of the scan blocks and sample
counts on both sides of a wavefront; `out=` slices, seeds, launch block sizes, the status word, inflation, the parameter block and
one pass from a mesh to deformed means."""
import numpy as np
import pytest
import torch

import gauss_init_ref as gr

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64                                        # bytes in front of and behind every output (keeps the 16-byte alignment)
FILL = 0xA5
FACES = [1, 2, 255, 256, 257, 513, 65537]         # 65537: 257 scan blocks, more than one pass of the second-level scan's workgroup
COUNTS = [1, 63, 64, 65, 1000]
OUTPUTS = ("points", "rotations", "faces", "face_id", "barys")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _guarded_samples(n, shift=0):
    """a SurfaceSamples whose tensors sit between guard bands; shift: extra bytes in front (4: the quaternion rows lose their
    16-byte alignment and take the scalar stores)"""
    from d3ga_amd.gauss_init import _FIELDS, SurfaceSamples
    bufs, views = [], []
    for name, c, dt in _FIELDS + (("status", 0, torch.int32),):
        rows = 1 if name == "status" else n
        nbytes = rows * max(c, 1) * 4
        buf = torch.full((nbytes + 2 * GUARD + shift,), FILL, dtype=torch.uint8, device=DEV)
        view = buf[GUARD + shift:GUARD + shift + nbytes].view(dt).view((rows, c) if c else (rows,))
        bufs.append((buf, shift))
        views.append(view)
    views[-1].zero_()
    return bufs, SurfaceSamples(*views)


def _bands_intact(bufs):
    return all(bool((b[:GUARD + s] == FILL).all()) and bool((b[-GUARD:] == FILL).all()) for b, s in bufs)


def _equal(got, want):
    for k in OUTPUTS:
        assert gr.same_bits(getattr(got, k).cpu().numpy(), want[k]), k
    assert int(got.status.item()) == want["status"]


_MESHES = {}


def _mesh(F):
    if F not in _MESHES:
        v, f = gr.random_mesh(F, F)
        mask = np.random.default_rng(F).random(F) < 0.5
        mask[F // 2] = True
        _MESHES[F] = (v, f, mask, _dev(v), _dev(f), _dev(mask))
    return _MESHES[F]


@pytest.mark.parametrize("masked", [False, True], ids=["all", "mask"])
@pytest.mark.parametrize("F", FACES)
def test_kernels_equal_the_host_build_bit_for_bit(F, masked):
    from d3ga_amd.gauss_init import sample_surface
    v, f, mask, dv, df, dmask = _mesh(F)
    for n in COUNTS:
        u = gr.uniforms(n, 7 * F + n)
        want = gr.host_sample(v, f, u, mask if masked else None)
        assert want["status"] == 0
        for shift in ((0, 4) if n in (1, 65) else (0,)):
            bufs, out = _guarded_samples(n, shift)
            assert (out.rotations.data_ptr() % 16 == 0) == (shift == 0)
            got = sample_surface(dv, df, n, face_mask=dmask if masked else None, uniforms=_dev(u), out=out)
            torch.cuda.synchronize()
            assert got is out and _bands_intact(bufs)
            _equal(out, want)


def test_converted_inputs_slices_and_seeds():
    from d3ga_amd.gauss_init import SurfaceSamples, sample_surface
    v, f, mask, dv, df, dmask = _mesh(513)
    # float32 vertices and int64 faces are converted once: the result is that of the float64 / int32 mesh they hold
    v32 = v.astype(np.float32)
    u = gr.uniforms(200, 9)
    _equal(sample_surface(_dev(v32), df.long(), 200, uniforms=_dev(u)), gr.host_sample(v32.astype(np.float64), f, u))
    _equal(sample_surface(v, f, 200, uniforms=u, face_mask=mask), gr.host_sample(v, f, u, mask))      # arrays are uploaded
    # two draws into one buffer equal the single calls
    both = SurfaceSamples.empty(300, DEV)
    ua, ub = gr.uniforms(100, 10), gr.uniforms(200, 11)
    sample_surface(dv, df, 100, uniforms=_dev(ua), out=both.rows(0, 100))
    sample_surface(dv, df, 200, uniforms=_dev(ub), face_mask=dmask, out=both.rows(100, 300))
    a, b = sample_surface(dv, df, 100, uniforms=_dev(ua)), sample_surface(dv, df, 200, uniforms=_dev(ub), face_mask=dmask)
    for k in OUTPUTS:
        assert torch.equal(getattr(both, k), torch.cat([getattr(a, k), getattr(b, k)]))
    assert both.check() is both and bool(dmask[both.face_id[100:].long()].all())
    # the same seed gives the same bytes twice, another seed gives other samples; seeded draws are torch.rand's
    s1, s2, s3 = (sample_surface(dv, df, 1000, seed=s) for s in (42, 42, 43))
    for k in OUTPUTS:
        assert torch.equal(getattr(s1, k), getattr(s2, k))
    assert not torch.equal(s1.points, s3.points)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(42)
    drawn = torch.rand((1000, 3), dtype=torch.float64, device=DEV, generator=gen)
    _equal(s1, gr.host_sample(v, f, drawn.cpu().numpy()))
    # independent of the launch block size
    for block in (64, 128, 256, 512, 1024):
        got = sample_surface(dv, df, 1000, uniforms=drawn, block=block)
        for k in OUTPUTS:
            assert torch.equal(getattr(got, k), getattr(s1, k)), (block, k)
    # area-weighted: the faces' shares of 200 000 samples follow their areas (binomial, 6 sigma)
    big = sample_surface(dv, df, 200000, seed=1)
    share = gr.face_areas(v, f) / gr.face_areas(v, f).sum()
    counts = np.bincount(big.face_id.cpu().numpy(), minlength=513)
    assert (np.abs(counts - 200000 * share) <= 6 * np.sqrt(200000 * share * (1 - share)) + 1).all()


def test_nothing_to_sample_from_is_a_flag():
    from d3ga_amd.gauss_init import sample_surface
    v, f, mask, dv, df, dmask = _mesh(257)
    u = gr.uniforms(70, 3)
    bufs, out = _guarded_samples(70)
    sample_surface(dv, df, 70, face_mask=torch.zeros_like(dmask), uniforms=_dev(u), out=out)
    torch.cuda.synchronize()
    assert _bands_intact(bufs)
    _equal(out, gr.host_sample(v, f, u, np.zeros(257, bool)))
    assert int(out.status.item()) == gr.STATUS_EMPTY and bool((out.face_id == -1).all()) and not bool(out.points.any())
    with pytest.raises(ValueError):
        out.check()
    # sticky: a good draw into the same buffer leaves the flag up, and writes its samples
    sample_surface(dv, df, 70, uniforms=_dev(u), out=out)
    assert int(out.status.item()) == gr.STATUS_EMPTY and gr.same_bits(out.points.cpu().numpy(), gr.host_sample(v, f, u)["points"])
    # a mesh without area
    flat = sample_surface(torch.zeros_like(dv), df, 5, seed=0)
    assert int(flat.status.item()) == gr.STATUS_EMPTY


@pytest.mark.parametrize("F", [1, 257, 3000])
def test_inflate_equals_the_host_build(F):
    """acos is the one library call of the rules, and the device's and the host's need not agree to the last bit: the bound per
    vertex is tests/gauss_init_ref.py::normals_bound (derived there); the inflated vertex adds |amount| times that and one
    rounding of its own.  Everything else must be the same bits: inflated == vertices + amount x the kernel's own normals."""
    from d3ga_amd import MeshTopology
    from d3ga_amd.gauss_init import inflate, vertex_normals_angle
    v, f, _, dv, df, _ = _mesh(F)
    amount = 0.03
    want_n, want_v = gr.host_normals(v, f, amount)
    normals = vertex_normals_angle(dv, df)
    moved = inflate(dv, MeshTopology(f), amount)
    assert normals.dtype == torch.float64 and moved.dtype == torch.float64 and tuple(moved.shape) == v.shape
    bound = gr.normals_bound(gr.vertex_normals_angle(v, f, want_condition=True)[1])
    dn = np.abs(normals.cpu().numpy() - want_n).max(1)
    dm = np.abs(moved.cpu().numpy() - want_v).max(1)
    print(f"{F} faces: normals differ by {dn.max():.3e}, inflated vertices by {dm.max():.3e}; the bounds reach {bound.max():.3e}")
    assert (dn <= bound).all()
    assert (dm <= amount * bound + np.spacing(np.abs(want_v).max(1))).all()
    assert torch.equal(moved, dv + amount * normals)
    assert torch.equal(inflate(dv.float(), df.long(), amount), inflate(dv.float().double(), df, amount))


def test_init_cage_parameters():
    from d3ga_amd.gauss_init import init_cage_parameters, sample_surface
    from d3ga_amd.tetra import knn_mean_dist2
    v, f, _, dv, df, _ = _mesh(513)
    s = sample_surface(dv, df, 3000, seed=5)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(9)
    p = init_cage_parameters(s.points, s.rotations, 64, 3, True, gen)
    shapes = {"colors_feat": (3000, 64), "rotation": (3000, 4), "scaling": (3000, 3), "opacities": (3000, 1), "features_dc": (3000, 1, 3),
              "features_rest": (3000, 15, 3)}
    assert list(p) == list(shapes)
    for k, shape in shapes.items():
        assert tuple(p[k].shape) == shape and p[k].dtype == torch.float32 and p[k].is_contiguous() and p[k].is_cuda, k
    assert torch.equal(p["rotation"], s.rotations) and p["rotation"].data_ptr() != s.rotations.data_ptr()
    want = torch.log(torch.sqrt(torch.clamp_min(knn_mean_dist2(s.points), 0.0000001)))
    assert torch.equal(p["scaling"], want[:, None].repeat(1, 3)) and bool(torch.isfinite(p["scaling"]).all())
    assert 0 <= float(p["colors_feat"].min()) and float(p["colors_feat"].max()) < 0.33 and float(p["colors_feat"].std()) > 0.05
    assert 0 <= float(p["features_dc"].min()) and float(p["features_dc"].max()) < 1 / 255 and not bool(p["features_rest"].any())
    assert torch.allclose(torch.sigmoid(p["opacities"]), torch.full((3000, 1), 0.2, device=DEV), atol=1e-6)
    gen.manual_seed(9)
    again = init_cage_parameters(s.points, s.rotations, 64, 3, True, gen)
    assert all(torch.equal(p[k], again[k]) for k in p)
    assert list(init_cage_parameters(s.points, s.rotations, 8, 0, False)) == ["colors_feat", "rotation", "scaling"]


def test_from_a_mesh_to_deformed_means():
    """sample_initial_points -> compute_bary -> cage_deform on a small synthetic cage: finite means inside the cage's box."""
    from types import SimpleNamespace
    from d3ga_amd.cage_deform import cage_deform, canonical_gradient
    from d3ga_amd.gauss_init import init_cage_parameters, sample_initial_points
    from d3ga_amd.synthetic import kuhn_cage
    from d3ga_amd.tetra import compute_bary
    rng = np.random.default_rng(3)
    lo, hi = np.array([-1.0, -1.0, -1.0]), np.array([1.0, 1.0, 1.0])
    cage_pts, tets = kuhn_cage(4, lo, hi, 0.1, rng)
    v, f = gr.random_mesh(400, 8)
    v = np.clip(v * 0.25, -0.7, 0.7)                         # well inside the cage, inflated or not
    labels = (np.arange(400) % 3).astype(np.int64)
    region = np.arange(400) < 40
    cages = {"body": dict(label_id=[-1], n_gaussians=900, n_under_gaussians=300, inflate=0.01), "face": dict(label_id=[-1], n_gaussians=200, inflate=0.0),
             "upper": dict(label_id=[1], n_gaussians=700, inflate=0.03)}
    config = SimpleNamespace(cages=cages)
    tp, tt = _dev(cage_pts), _dev(tets)
    for name, total in (("body", 1200), ("face", 200), ("upper", 700)):
        cfg = dict(cages[name], cage_name=name)
        points, rotations, faces, barys = sample_initial_points(_dev(v), _dev(f), cfg, config, labels, face_mask=region, seed=11)
        again = sample_initial_points(_dev(v), _dev(f), cfg, config, labels, face_mask=region, seed=11)
        assert all(torch.equal(a, b) for a, b in zip((points, rotations, faces, barys), again))
        assert tuple(points.shape) == (total, 3) and tuple(rotations.shape) == (total, 4) and tuple(faces.shape) == (total, 3)
        assert faces.dtype == torch.int32 and tuple(barys.shape) == (total, 3) and torch.allclose(barys.sum(1), torch.ones(total, device=DEV), atol=1e-4)
        if name == "face":
            ids = {tuple(r) for r in f[region].tolist()}
            assert all(tuple(r) in ids for r in faces.cpu().tolist())
        tet_barys, tetra_id, active = compute_bary(points, tp[tt.long()])
        assert bool(active.all())
        p = init_cage_parameters(points, rotations, 8, 3)
        grad = canonical_gradient(tp, tt, tetra_id)
        for moved in (tp, tp * 1.1 + 0.05):
            means, cov6 = cage_deform(moved, tt, tetra_id, tet_barys, grad, torch.exp(p["scaling"]), torch.nn.functional.normalize(p["rotation"]))
            assert bool(torch.isfinite(means).all()) and bool(torch.isfinite(cov6).all())
            assert bool((means >= moved.amin(0)).all()) and bool((means <= moved.amax(0)).all())
        assert torch.allclose(cage_deform(tp, tt, tetra_id, tet_barys, grad, torch.exp(p["scaling"]), torch.nn.functional.normalize(p["rotation"]))[0], points,
                              atol=1e-4)
