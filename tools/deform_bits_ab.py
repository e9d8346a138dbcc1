#!/usr/bin/env python3
"""Bit-for-bit comparison of the cage-side operators between two checkouts (or two builds of the library).

Only the public Python operators are called (cage_deform, lbs_cage, lbs_cage_deform, fem_energy), so the same file runs in
either tree:

    python tools/deform_bits_ab.py digest bits_a.json          # in checkout A
    python tools/deform_bits_ab.py digest bits_b.json          # in checkout B
    python tools/deform_bits_ab.py compare bits_a.json bits_b.json      # exit 1 on any differing digest

`digest` stores a SHA-256 of every output and of every returned gradient of
  cage_deform      the first P Gaussians of scene C1, P in {0, 1, 255, 257, 10000}, sorted by tetrahedron and shuffled, with and
                   without delta_barys, scale_activation None / "exp", the canonical gradient per Gaussian / per tetrahedron, under
                   both settings of the vertex-gradient route (_merge_policy);
  lbs_cage, lbs_cage_deform   (K, J) = (4, 55) and (8, 160), with and without delta + Rh + Th, with and without pose gradients,
                   lbs_cage_deform also with a gradient that reaches the returned tetpoints through fem_energy, and with P == 0,
                   V == 1 and both (a backward that the library refuses is recorded by its status code); lbs_cage also with V == 1;
  cage_deform also with P == 0;
  a captured graph of lbs_cage_deform + lbs_cage, forward and backward, replayed twice with new inputs.
fem_energy's backward adds with float atomics, so the energies are weighted over tetrahedra that share no vertex: every vertex
then receives at most one non-zero term and the sum does not depend on the order.
"""
import hashlib
import itertools
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def digest(out_path):
    import numpy as np
    import torch
    from d3ga_amd import _lib, cage_deform as cd, synthetic as syn
    dev = torch.device("cuda")
    d = lambda t: None if t is None else t.to(dev)
    sc = syn.make_scene("C1")
    canon, tetras = sc["canon_points"], sc["tetras"]
    V, T, P_all = canon.shape[0], tetras.shape[0], sc["tetra_id"].shape[0]
    gen = torch.Generator().manual_seed(11)
    rnd = lambda *shape: torch.randn(*shape, generator=gen)
    tetpoints = canon + 0.01 * rnd(V, 3)
    grad_tet = cd.canonical_gradient_per_tet(canon, tetras).contiguous()
    shuffle = torch.randperm(P_all, generator=gen)
    g_means_all, g_cov6_all, dbary_all = rnd(P_all, 3), rnd(P_all, 6), 0.01 * rnd(P_all, 4)
    Dn_inv = grad_tet + 0.01 * rnd(T, 3, 3)
    used, e_weight = np.zeros(V, bool), torch.zeros(T)            # tetrahedra that share no vertex (see the module docstring)
    for t, vid in enumerate(tetras.tolist()):
        if not used[vid].any():
            used[vid] = True
            e_weight[t] = 0.5 + (t % 7)
    cases = {}

    def grads_of(loss, named):
        named = {k: v for k, v in named.items() if v is not None and v.requires_grad}
        try:
            got = torch.autograd.grad(loss, list(named.values()), allow_unused=True)
        except _lib.D3GAError as e:                      # a refusal is part of the behaviour: its status is the digest
            return {"d_*": "refused with " + re.search(r"status -?\d+", str(e)).group(0)}
        return {"d_" + k: ("none" if g is None else sha(g)) for k, g in zip(named, got)}

    def deform_inputs(P, shuffled, with_db, act, per_tet):
        sel = (shuffle[:P] if shuffled else torch.arange(P))
        tid = sc["tetra_id"][sel].contiguous()
        leaf = lambda t: d(t.contiguous()).requires_grad_(True)
        scales = sc["scaling"][sel] if act == "exp" else sc["scaling"][sel].exp()
        grad = grad_tet if per_tet else grad_tet[tid.long()].contiguous()
        return dict(tetras=d(tetras), tetra_id=d(tid), barys=leaf(sc["barys"][sel]), grad=d(grad), scales=leaf(scales),
                    rotations=leaf(sc["rotation"][sel]), delta_barys=leaf(dbary_all[sel]) if with_db else None,
                    g_means=d(g_means_all[sel].contiguous()), g_cov6=d(g_cov6_all[sel].contiguous()), per_tet=per_tet, act=act)

    # ---- cage_deform
    for P, shuffled, with_db, act, per_tet, merged in itertools.product((0, 1, 255, 257, 10000), (False, True), (False, True), (None, "exp"),
                                                                        (False, True), (True, False)):
        a = deform_inputs(P, shuffled, with_db, act, per_tet)
        tp = d(tetpoints).requires_grad_(True)
        cd._merge_policy["enabled"] = merged
        try:
            means, cov6 = cd.cage_deform(tp, a["tetras"], a["tetra_id"], a["barys"], a["grad"], a["scales"], a["rotations"],
                                         delta_barys=a["delta_barys"], scale_activation=act, gradient_per_tet=per_tet)
            out = {"means": sha(means), "cov6": sha(cov6)}
            out.update(grads_of((means * a["g_means"]).sum() + (cov6 * a["g_cov6"]).sum(),
                                dict(tetpoints=tp, barys=a["barys"], scales=a["scales"], rotations=a["rotations"], delta_barys=a["delta_barys"])))
        finally:
            cd._merge_policy["enabled"] = True
        cases["cage_deform/P%d/%s/db%d/%s/%s/%s" % (P, "shuffled" if shuffled else "sorted", with_db, act or "plain",
                                                   "per_tet" if per_tet else "per_gaussian", "merge" if merged else "corners")] = out

    # ---- lbs_cage, lbs_cage_deform
    for K, J in ((4, 55), (8, 160)):
        rng = np.random.default_rng(100 + J)
        joint_pos, A = syn.make_skeleton(J, rng)
        idx, w = syn.skin_weights(canon.numpy(), joint_pos, K)
        Rh0 = torch.from_numpy(syn.rodrigues(np.array([0.3, -0.2, 0.1]))).float()
        for extras, pose in itertools.product((False, True), (False, True)):
            def skin_inputs(n_vertices):
                leaf = lambda t, on=True: d(t.contiguous()).requires_grad_(on)
                return dict(template=leaf(canon[:n_vertices]), delta=leaf(sc["delta_node"][:n_vertices]) if extras else None,
                            joint_mats=leaf(torch.from_numpy(A), pose), skin_idx=d(torch.from_numpy(idx[:n_vertices].copy())),
                            skin_w=d(torch.from_numpy(w[:n_vertices].copy())), Rh=leaf(Rh0, pose) if extras else None,
                            Th=leaf(torch.tensor([0.1, -0.2, 0.3]), pose) if extras else None)

            def skin_leaves(s):
                return dict(template=s["template"], delta=s["delta"], joint_mats=s["joint_mats"], Rh=s["Rh"], Th=s["Th"])
            tag = "K%d_J%d/%s/%s" % (K, J, "delta_Rh_Th" if extras else "bare", "pose" if pose else "nopose")
            for nv in (V, 1):
                s = skin_inputs(nv)
                out = cd.lbs_cage(s["template"], s["delta"], s["joint_mats"], s["skin_idx"], s["skin_w"], s["Rh"], s["Th"])
                res = {"out": sha(out)}
                res.update(grads_of((out * d(g_means_all[:nv])).sum(), skin_leaves(s)))
                cases["lbs_cage/%s/V%d" % (tag, nv)] = res
            for fem, (P, nv) in itertools.product((False, True), ((10000, V), (0, V), (300, 1), (0, 1))):
                s = skin_inputs(nv)
                a = deform_inputs(P, True, True, "exp", True)
                if nv == 1:                              # one vertex: one collapsed tetrahedron, its matrices given
                    a.update(tetras=torch.zeros(1, 4, dtype=torch.int32, device=dev), tetra_id=torch.zeros(P, dtype=torch.int32, device=dev),
                             grad=d(grad_tet[:1].contiguous()))
                means, cov6, tp = cd.lbs_cage_deform(s["template"], s["delta"], s["joint_mats"], s["skin_idx"], s["skin_w"], a["tetras"],
                                                     a["tetra_id"], a["barys"], a["grad"], a["scales"], a["rotations"],
                                                     delta_barys=a["delta_barys"], scale_activation="exp", gradient_per_tet=True,
                                                     Rh=s["Rh"], Th=s["Th"])
                res = {"means": sha(means), "cov6": sha(cov6), "tetpoints": sha(tp)}
                loss = (means * a["g_means"]).sum() + (cov6 * a["g_cov6"]).sum()
                if fem:
                    n_t = a["tetras"].shape[0]
                    energy = cd.fem_energy(tp, a["tetras"], d(Dn_inv[:n_t].contiguous()))
                    res["energy"] = sha(energy)
                    loss = loss + (energy * d(e_weight[:n_t])).sum()
                leaves = skin_leaves(s)
                leaves.update(barys=a["barys"], scales=a["scales"], rotations=a["rotations"], delta_barys=a["delta_barys"])
                res.update(grads_of(loss, leaves))
                cases["lbs_cage_deform/%s/P%d_V%d/%s" % (tag, P, nv, "fem" if fem else "nofem")] = res

    # ---- a captured step (forward + backward of both skinned operators in one graph), replayed with new inputs
    for pose in (False, True):
        rng = np.random.default_rng(7)
        joint_pos, A = syn.make_skeleton(55, rng)
        idx, w = syn.skin_weights(canon.numpy(), joint_pos, 4)
        a = deform_inputs(10000, False, True, "exp", False)
        leaf = lambda t, on=True: d(t.contiguous()).requires_grad_(on)
        tmpl, dl, A_s, Th_s = d(canon), leaf(sc["delta_node"]), leaf(torch.from_numpy(A), pose), leaf(torch.tensor([0.1, -0.2, 0.3]), pose)
        sidx, sw, g_tp = d(torch.from_numpy(idx)), d(torch.from_numpy(w)), d(g_means_all[:V].contiguous())
        leaves = [dl, a["barys"], a["scales"], a["rotations"], a["delta_barys"]] + ([A_s, Th_s] if pose else [])

        def step():
            means, cov6, tp = cd.lbs_cage_deform(tmpl, dl, A_s, sidx, sw, a["tetras"], a["tetra_id"], a["barys"], a["grad"], a["scales"],
                                                 a["rotations"], delta_barys=a["delta_barys"], scale_activation="exp", Th=Th_s)
            tp2 = cd.lbs_cage(tmpl, dl, A_s, sidx, sw, None, Th_s)
            loss = (means * a["g_means"]).sum() + (cov6 * a["g_cov6"]).sum() + (tp * g_tp).sum() + (tp2 * tp2).sum()
            return (means, cov6, tp, tp2) + torch.autograd.grad(loss, leaves)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                step()
        torch.cuda.current_stream().wait_stream(side)
        gph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gph):
            cap = step()
        for k in range(2):
            with torch.no_grad():
                dl.copy_(d(sc["delta_node"] * (k + 2)))
                A_s.copy_(d(torch.from_numpy(syn.pose_matrices(joint_pos, np.random.default_rng(20 + k)))))
            gph.replay()
            torch.cuda.synchronize()
            cases["captured/%s/replay%d" % ("pose" if pose else "nopose", k)] = {"out%d" % i: sha(t) for i, t in enumerate(cap)}
    torch.cuda.synchronize()
    total = hashlib.sha256(json.dumps(cases, sort_keys=True).encode()).hexdigest()
    json.dump({"library": _lib.library_path(), "abi": _lib.ABI_VERSION, "cases": cases, "summary": total}, open(out_path, "w"), indent=1)
    print("%d cases, %d digests, summary %s (ABI %d)" % (len(cases), sum(len(c) for c in cases.values()), total, _lib.ABI_VERSION))


def compare(a_path, b_path):
    a, b = json.load(open(a_path)), json.load(open(b_path))
    print("A: ABI %s, %s, summary %s\nB: ABI %s, %s, summary %s" % (a["abi"], a["library"], a["summary"], b["abi"], b["library"], b["summary"]))
    bad = 0
    if sorted(a["cases"]) != sorted(b["cases"]):
        print("DIFFERENT CASE SETS")
        bad += 1
    for name in sorted(a["cases"]):
        ca, cb = a["cases"][name], b["cases"].get(name, {})
        diff = [k for k in sorted(set(ca) | set(cb)) if ca.get(k) != cb.get(k)]
        bad += len(diff)
        if diff:
            print("%-70s DIFFERS in %s" % (name, ", ".join(diff)))
    print("%d cases, %d digests, %d differing" % (len(a["cases"]), sum(len(c) for c in a["cases"].values()), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "digest":
        sys.exit(digest(sys.argv[2]))
    if len(sys.argv) >= 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    sys.exit(__doc__)
