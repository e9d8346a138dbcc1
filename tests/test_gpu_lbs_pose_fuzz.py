"""Randomised pose gradients of the cage skinning against float64 (oracle.deform): V in 1..4000, J in 1..160, K in {1,2,3,4,8,24},
optional delta / Rh / Th, any subset of requested gradients, lbs_cage on even seeds and lbs_cage_deform (random tetrahedra over
the vertices, a second route into the posed vertices) on odd ones.  Bars as tests/test_gpu_lbs_pose_grad.py.  6 seeds by
default; D3GA_LBS_POSE_FUZZ_N=500 is the campaign (tools/gpu_campaigns.sh)."""
import os

import pytest
import torch

from oracle import deform as od
from test_gpu_lbs_pose_grad import DEV, check_pose, excess, pose_floors, random_rotation

pytestmark = pytest.mark.gpu
N = int(os.environ.get("D3GA_LBS_POSE_FUZZ_N", "6"))


@pytest.mark.parametrize("seed", range(N))
def test_lbs_pose_fuzz(seed):
    from d3ga_amd.cage_deform import lbs_cage, lbs_cage_deform
    g = torch.Generator().manual_seed(1000 + seed)
    ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))
    V, J, K = ri(1, 4000), ri(1, 160), [1, 2, 3, 4, 8, 24][ri(0, 5)]
    fused = seed % 2 == 1 and V >= 4
    idx = torch.randint(0, J, (V, K), generator=g)
    if ri(0, 2) == 0:                                       # skew: one joint carries most entries (SMPL-X's pelvis / spine)
        idx[torch.rand(V, K, generator=g) < 0.7] = ri(0, J - 1)
    idx = idx.to(torch.int32)
    w = torch.rand(V, K, generator=g)
    w[torch.rand(V, K, generator=g) < 0.2] = 0.0
    A = torch.eye(4).repeat(J, 1, 1) + 0.3 * torch.randn(J, 4, 4, generator=g)
    tmpl = torch.randn(V, 3, generator=g)
    delta = 0.05 * torch.randn(V, 3, generator=g) if ri(0, 1) else None
    Rh = random_rotation(g) if ri(0, 1) else None
    Th = torch.randn(3, generator=g) if ri(0, 1) else None
    want = [True] + [bool(ri(0, 1)) for _ in range(3)]     # joint_mats always; delta, Rh, Th at random
    lv = lambda t, on: None if t is None else (t.clone().to(DEV).requires_grad_(True) if on else t.to(DEV))
    Al, dl, Rl, Tl = lv(A, True), lv(delta, want[1]), lv(Rh, want[2]), lv(Th, want[3])
    if not fused:
        gout = torch.randn(V, 3, generator=g)
        out = lbs_cage(tmpl.to(DEV), dl, Al, idx.to(DEV), w.to(DEV), Rl, Tl)
        (out * gout.to(DEV)).sum().backward()
        gv = gout
        d = lambda t, on: None if t is None else t.double().requires_grad_(on)
        tl, dd, Ad, Rd, Td = d(tmpl, False), d(delta, want[1]), d(A, True), d(Rh, want[2]), d(Th, want[3])
        (od.lbs_cage(tl, dd, Ad, idx.long(), w.double(), Rd, Td) * gout.double()).sum().backward()
    else:
        T, P = ri(1, 2 * V), ri(1, 3000)
        tetras = torch.stack([torch.randperm(V, generator=g)[:4] for _ in range(T)]).to(torch.int32)
        tid = torch.sort(torch.randint(0, T, (P,), generator=g))[0].to(torch.int32)
        barys = torch.rand(P, 4, generator=g)
        cg = torch.eye(3) + 0.3 * torch.randn(P, 3, 3, generator=g)
        scales, rots = 0.1 + torch.rand(P, 3, generator=g), torch.randn(P, 4, generator=g)
        gm, gc, gt = torch.randn(P, 3, generator=g), torch.randn(P, 6, generator=g), torch.randn(V, 3, generator=g)
        dv = lambda t: t.to(DEV)
        m, c, tp = lbs_cage_deform(tmpl.to(DEV), dl, Al, idx.to(DEV), w.to(DEV), dv(tetras), dv(tid), dv(barys), dv(cg), dv(scales),
                                   dv(rots), Rh=Rl, Th=Tl, gradient_per_tet=False)
        ((m * gm.to(DEV)).sum() + (c * gc.to(DEV)).sum() + (tp * gt.to(DEV)).sum()).backward()
        d = lambda t, on: None if t is None else t.double().requires_grad_(on)
        tl, dd, Ad, Rd, Td = d(tmpl, False), d(delta, want[1]), d(A, True), d(Rh, want[2]), d(Th, want[3])
        tpd = od.lbs_cage(tl, dd, Ad, idx.long(), w.double(), Rd, Td)
        tpv = tpd.detach().requires_grad_(True)
        md, cd = od.cage_deform(tpv, tetras.long(), tid.long(), barys.double(), cg.double(), scales.double(), rots.double())
        ((md * gm.double()).sum() + (cd * gc.double()).sum() + (tpv * gt.double()).sum()).backward()
        gv = tpv.grad
        tpd.backward(gv)
    torch.cuda.synchronize()
    ref = dict(A=Ad.grad, Rh=None if Rd is None or not want[2] else Rd.grad, Th=None if Td is None or not want[3] else Td.grad)
    got = dict(A=Al.grad, Rh=None if Rl is None or not want[2] else Rl.grad, Th=None if Tl is None or not want[3] else Tl.grad)
    check_pose(got, ref, pose_floors(tmpl, delta, A, idx, w, Rh, gv), f"seed {seed} V={V} J={J} K={K} fused={fused}")
    if dl is not None and want[1] and not fused:       # the fused operator's offset gradient is pinned by the older tests
        assert excess(dl.grad.cpu(), dd.grad) <= 1.0
