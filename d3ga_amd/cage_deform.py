"""Autograd ops of the cage side of the hot path: LBS of cage vertices, fused tet-cage deformation, FEM energy.

Host-side mirror of the reference's per-frame tensor program:
    lib/smplman.py:155-171        -> lbs_cage
    models/cage_net.py:218-230    -> cage_deform      (replaces tetpoints[tetra_faces], compute_def_grad,
                                                        J S J^T, strip_symmetric and the bary einsum)
    lib/cage.py:349-361           -> fem_energy
All three call hand-written gfx950 kernels through the C ABI (include/d3ga.h); GPU tensors only.
"""
import ctypes
import warnings

import torch

from . import _lib
from ._lib import check, dptr, require_cuda, stream_handle


def _f32c(t):
    if t is None:
        return None
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


class StorageCache:
    """Values derived from tensors that stay put (index buffers, templates), built once: keyed by every source's (data_ptr,
    _version, shape, dtype) and `extra`.  An entry pins its sources, so their addresses cannot be recycled while it lives;
    beyond `limit` entries the cache is emptied."""

    def __init__(self, limit=64):
        self.limit, self.entries = limit, {}

    def get(self, sources, extra, build):
        key = tuple((t.data_ptr(), t._version, tuple(t.shape), t.dtype) for t in sources) + (extra,)
        hit = self.entries.get(key)
        if hit is None:
            value = build()
            if len(self.entries) > self.limit:
                self.entries.clear()
            hit = self.entries[key] = (value, sources)
        return hit[0]


_i32_cache, _adjacency_cache, _plan_cache, _pose_plan_cache = StorageCache(), StorageCache(), StorageCache(), StorageCache()


def _i32c(t):
    """int32 contiguous view of an index buffer.  The reference registers int64 buffers (lib/cage.py:331-337); their
    int32 copies are cached so that per-frame calls neither convert again nor defeat the adjacency cache below."""
    if t.dtype == torch.int32 and t.is_contiguous():
        return t
    return _i32_cache.get((t,), None, lambda: t.to(torch.int32).contiguous())


def vertex_adjacency(tetras, tetra_id, n_vertices):
    """Static CSR adjacency vertex -> items (4*gaussian + corner) of a cage binding; built once and cached.
    (tetra_id / tetras are buffers fixed at initialisation, lib/cage.py:331-337.)"""
    def build():
        with torch.no_grad():
            vid = tetras.long()[tetra_id.long()].reshape(-1)                    # (4P,) vertex of item 4*i + corner
            order = torch.sort(vid, stable=True)[1]
            counts = torch.bincount(vid, minlength=n_vertices)
            start = torch.zeros(n_vertices + 1, dtype=torch.int64, device=vid.device)
            start[1:] = torch.cumsum(counts, 0)
            return start.to(torch.int32).contiguous(), order.to(torch.int32).contiguous()
    return _adjacency_cache.get((tetras, tetra_id), n_vertices, build)


_MERGE_BLOCK = 256        # = kBlock of csrc/deform.hip: the Gaussians of one workgroup
# enabled = False: per-corner gradient records + a gather over all 4P items (rounds 1-3; kept for A/B runs and tests)
_merge_policy = {"enabled": True}


def merge_plan(tetras, tetra_id, n_vertices):
    """Static plan of the block-merged backward (D3GA_DEFORM_ROUTE_MERGE), built once per binding and cached:
    -> dict(item_pos (P,4) int16-as-uint16, seg_ptr (blocks+1) int32, seg_begin (segments) uint16 stored as int16,
            vert_start (V+1) int32, vert_parts (segments) int32, n_segments).
    Items are (Gaussian, corner) pairs, 1024 per workgroup of 256 consecutive Gaussians; inside a workgroup they are ordered
    by cage vertex (stable), a SEGMENT is a run of equal vertex, and every segment's sum becomes one partial."""
    def build():
        with torch.no_grad():
            dev = tetra_id.device
            P = tetra_id.shape[0]
            per = 4 * _MERGE_BLOCK
            vid = tetras.long()[tetra_id.long()].reshape(-1)                    # (4P,) vertex of item 4 i + corner
            item = torch.arange(4 * P, device=dev)
            blk = item // per
            order = torch.sort(blk * n_vertices + vid, stable=True)[1]          # items by (workgroup, vertex), stable
            inv = torch.empty_like(order)
            inv[order] = item
            item_pos = (inv - blk * per).to(torch.int16).reshape(P, 4).contiguous()      # < 1024: the bit pattern of a uint16
            key_sorted = (blk * n_vertices + vid)[order]
            first = torch.ones(4 * P, dtype=torch.bool, device=dev)
            first[1:] = key_sorted[1:] != key_sorted[:-1]
            seg_first = torch.nonzero(first).reshape(-1)                        # sorted index of every segment's first item
            seg_key = key_sorted[seg_first]
            seg_blk, seg_vid = seg_key // n_vertices, seg_key % n_vertices
            nb = (P + _MERGE_BLOCK - 1) // _MERGE_BLOCK
            seg_ptr = torch.zeros(nb + 1, dtype=torch.int64, device=dev)
            seg_ptr[1:] = torch.cumsum(torch.bincount(seg_blk, minlength=nb), 0)
            seg_begin = (seg_first - seg_blk * per).to(torch.int16).contiguous()
            order2 = torch.sort(seg_vid, stable=True)[1]
            vstart = torch.zeros(n_vertices + 1, dtype=torch.int64, device=dev)
            vstart[1:] = torch.cumsum(torch.bincount(seg_vid, minlength=n_vertices), 0)
            return dict(item_pos=item_pos, seg_ptr=seg_ptr.to(torch.int32).contiguous(), seg_begin=seg_begin,
                        vert_start=vstart.to(torch.int32).contiguous(), vert_parts=order2.to(torch.int32).contiguous(),
                        n_segments=int(seg_first.numel()))
    return _plan_cache.get((tetras, tetra_id), n_vertices, build)


def _deform_in(tetpoints, tetras, tetra_id, barys, canon_grad, scales, rotations, delta_barys, flags):
    """struct d3ga_cage_deform_in (delta_barys None -> NULL)."""
    return _lib.CageDeformIn(P=barys.shape[0], V=tetpoints.shape[0], flags=flags, tetpoints=dptr(tetpoints), tetras=dptr(tetras),
                             tetra_id=dptr(tetra_id), barys=dptr(barys), canon_grad=dptr(canon_grad), scales=dptr(scales),
                             rots=dptr(rotations), delta_barys=dptr(delta_barys))


def _deform_fwd(st, dev):
    means = torch.empty((st.P, 3), dtype=torch.float32, device=dev)
    cov6 = torch.empty((st.P, 6), dtype=torch.float32, device=dev)
    check(_lib.lib().d3ga_cage_deform_fwd(ctypes.byref(st), dptr(means), dptr(cov6), stream_handle()), "d3ga_cage_deform_fwd")
    return means, cov6


def _deform_saved(saved, has_delta_barys):
    """The eight tensors both nodes save first, by name (an empty tensor stands for a missing delta_barys)."""
    names = ("tetpoints", "tetras", "tetra_id", "barys", "canon_grad", "scales", "rotations", "delta_barys")
    inputs = dict(zip(names, saved[:8]))
    if not has_delta_barys:
        inputs["delta_barys"] = None
    return inputs


def _route(tetras, tetra_id, P, V, dev, merged, records=None):
    """struct d3ga_cage_deform_route over the static binding, with fresh records unless given: the block-merge plan (`merged`) or
    the per-corner records.  -> (struct, records, merged); the tensors must stay alive until the launches are queued."""
    new = lambda n: torch.empty((n, 3), dtype=torch.float32, device=dev)
    if merged:
        plan = merge_plan(tetras, tetra_id, V)
        records = new(max(plan["n_segments"], 1)) if records is None else records
        return _lib.CageDeformRoute(kind=_lib.DEFORM_ROUTE_MERGE, n_segments=plan["n_segments"], item_pos=dptr(plan["item_pos"]),
                                    seg_ptr=dptr(plan["seg_ptr"]), seg_begin=dptr(plan["seg_begin"]),
                                    vert_start=dptr(plan["vert_start"]), vert_items=dptr(plan["vert_parts"]),
                                    records=dptr(records)), records, True
    vstart, vitems = vertex_adjacency(tetras, tetra_id, V)
    records = new(4 * P) if records is None else records
    return _lib.CageDeformRoute(kind=_lib.DEFORM_ROUTE_CORNERS, vert_start=dptr(vstart), vert_items=dptr(vitems),
                                records=dptr(records)), records, False


def _route_choice(P, want_vertices, skinned):
    """Which route a backward takes -> None (no vertex gradient wanted) | True (block merge) | False (per-corner records).
    (P == 0 without the skinning tail: the library zeroes g_tetpoints without a route.)"""
    if skinned or (want_vertices and P > 0 and _merge_policy["enabled"]):
        return True
    return False if (want_vertices and P > 0) else None


def _deform_call(entry, inputs, flags, g_means, g_cov6, g_b, g_s, g_r, *, want_tetpoints, skin, pose, route_records=None):
    """One call of d3ga_cage_deform_bwd (`entry`) or d3ga_cage_deform_bwd_tail (on `route_records` = (records, merged) that a
    render's backward filled) -> (g_tetpoints | g_delta | None, (gA, gRh, gTh) | None, the route's records | None)."""
    tetras, tetra_id = inputs["tetras"], inputs["tetra_id"]
    st = _deform_in(flags=flags, **inputs)
    P, V, dev = st.P, st.V, inputs["barys"].device
    g_v = torch.empty((V, 3), dtype=torch.float32, device=dev) if (want_tetpoints or skin is not None) else None
    grads = _lib.CageDeformGrads(g_means=dptr(g_means), g_cov6=dptr(g_cov6), g_tetpoints=dptr(None if skin is not None else g_v),
                                 g_barys=dptr(g_b), g_scales=dptr(g_s), g_rots=dptr(g_r))
    route = tail = pose_st = pose_out = records = None
    if route_records is not None:
        route, records, _ = _route(tetras, tetra_id, P, V, dev, route_records[1], route_records[0])
    else:
        merged = _route_choice(P, g_v is not None, skin is not None)
        if merged is not None:
            route, records, _ = _route(tetras, tetra_id, P, V, dev, merged)
    if skin is not None:
        g_extra = _f32c(skin["g_extra"])
        tail = _lib.CageDeformSkin(K=skin["skin_w"].shape[1], joint_mats=dptr(skin["joint_mats"]), skin_idx=dptr(skin["skin_idx"]),
                                   skin_w=dptr(skin["skin_w"]), Rh=dptr(skin["Rh"]), g_tetpoints_extra=dptr(g_extra), g_delta=dptr(g_v))
        if pose is not None:
            plan_p = lbs_pose_plan(skin["skin_idx"], skin["joint_mats"].shape[0])
            pose_st, pose_out, scratch = _pose_grad_struct(plan_p, V, 1, pose["template"], pose["delta"], dev)
    ref = lambda x: None if x is None else ctypes.byref(x)
    check(getattr(_lib.lib(), entry)(ctypes.byref(st), ctypes.byref(grads), ref(route), ref(tail), ref(pose_st), stream_handle()), entry)
    return g_v, pose_out, records


def _deform_bwd(inputs, flags, g_means, g_cov6, *, want_tetpoints=False, want_barys, want_scales, want_rotations, skin=None, pose=None,
                deposit=None):
    """The one call of d3ga_cage_deform_bwd.  inputs: _deform_saved(...); want_*: which gradients to form.
    skin = dict(joint_mats, skin_idx, skin_w, Rh | None, g_extra | None): the skinning tail, whose g_delta stands in for the vertex
    gradient; pose = dict(template, delta | None) adds the pose gradients to it.
    deposit: what a claimed render's backward left on the node (render fusion, below) -- the per-Gaussian gradients and the
    route's records of the render's share.  Without incoming gradients only the tails run, on the deposited records
    (d3ga_cage_deform_bwd_tail); with incoming gradients (a second consumer of the node's outputs) the kernel runs on them as
    always and the deposit's share is added: the backward is linear.
    -> dict(vertices = g_tetpoints | g_delta, barys, scales, rotations, pose = (gA, gRh, gTh)), None where not wanted."""
    P, dev = inputs["barys"].shape[0], inputs["barys"].device
    wants_v = want_tetpoints or skin is not None

    def tail_of_deposit(skin):
        if not wants_v or deposit["records"] is None:
            return None, None
        return _deform_call("d3ga_cage_deform_bwd_tail", inputs, flags, None, None, None, None, None, want_tetpoints=want_tetpoints,
                            skin=skin, pose=pose, route_records=(deposit["records"], deposit["merged"]))[:2]
    if deposit is not None and g_means is None and g_cov6 is None:
        _last_path[0] = "fused-tail"
        g_v, pose_out = tail_of_deposit(skin)
        return dict(vertices=g_v, barys=deposit["barys"], scales=deposit["scales"], rotations=deposit["rotations"], pose=pose_out)

    def new(n, c, on=True):
        return torch.empty((n, c), dtype=torch.float32, device=dev) if on else None
    g_means = torch.zeros((P, 3), device=dev) if g_means is None else _f32c(g_means)
    g_cov6 = torch.zeros((P, 6), device=dev) if g_cov6 is None else _f32c(g_cov6)
    g_b, g_s, g_r = new(P, 4, want_barys), new(P, 3, want_scales), new(P, 4, want_rotations)
    g_v, pose_out, _ = _deform_call("d3ga_cage_deform_bwd", inputs, flags, g_means, g_cov6, g_b, g_s, g_r, want_tetpoints=want_tetpoints,
                                    skin=skin, pose=pose)
    _last_path[0] = "kernel" if deposit is None else "kernel+deposit"
    if deposit is not None:
        deposit["binding"]._render_fusion_demoted = _fusion["epoch"]
        # the render's share: its per-Gaussian gradients as deposited, its vertex / pose gradients from the tails on its records
        # (g_extra has joined above, once)
        d_v, d_pose = tail_of_deposit(None if skin is None else dict(skin, g_extra=None))
        for mine, theirs in ((g_b, deposit["barys"]), (g_s, deposit["scales"]), (g_r, deposit["rotations"]), (g_v, d_v)):
            if mine is not None and theirs is not None:
                mine.add_(theirs)
        if pose_out is not None and d_pose is not None:
            for mine, theirs in zip(pose_out, d_pose):
                mine.add_(theirs)
    return dict(vertices=g_v, barys=g_b, scales=g_s, rotations=g_r, pose=pose_out)


# ------------------------------------------------------------------------------------------------------------
# render fusion: the per-Gaussian part of this backward as the tail of the rasterizer's per-Gaussian backward
# ------------------------------------------------------------------------------------------------------------
# When a render's means3D and cov3D_precomp ARE the two outputs of one deform node (models/cage_net.py:213-230 feeding the
# renderer), the rasterizer's backward need not write dL/dmeans3D and dL/dcov3D for this node to read back: its per-Gaussian kernel
# runs the deform backward on them while they are in registers (d3ga_raster_*_deform).  The handshake: renderer.render CLAIMS the
# node before its operator is applied (claim_for_render); the claimed render's backward fills the node's per-Gaussian gradients
# and route records (fused_tail_structs) and DEPOSITS them on the node, returning no gradient for the two tensors; the node's
# backward then runs only its tails on the deposit -- or, when another consumer of its outputs did send gradients, its kernel
# on those and adds the deposit.  One render per node and forward pass: a second render of the same package (the silhouette pass of
# models/trainer.py:102-110) goes the usual way AND revokes the first one's claim -- its gradients make the node run its kernel
# anyway, and kernel + tails on a deposit + the sums cost more launches than the fusion saves.  Both renders then take the
# two-kernel path, as with fusion off.  The same holds for any other consumer of the node's outputs that sends gradients (view
# directions for a colour network): that cannot be known when the render claims, so a binding whose node once ran "kernel+deposit"
# is DEMOTED -- not claimed again until set_render_fusion() is called -- and a training loop pays for it in its first step only
# (the warm-up steps of a graph capture included: the captured step is then the two-kernel one).  The mark is an attribute of the
# binding's `tetra_id` tensor (the int32 buffer the operator was handed, or its cached int32 copy): it lives and dies with it.
_fusion = {"enabled": True, "epoch": 0}      # epoch: marks of an earlier one no longer count
_last_path = [None]
_REVOKED = "revoked"      # node.claimed: False | the key of the claiming render's token | _REVOKED (until the node's backward clears it)


def set_render_fusion(enabled):
    """Switch the render fusion (on by default).  Off: every backward takes the two-kernel path.  Either way demoted bindings
    (see above) are re-armed."""
    _fusion["enabled"] = bool(enabled)
    _fusion["epoch"] += 1


def last_backward_path():
    """How the most recent deform backward of this process ran: "fused-tail" (only the tails, on a render's deposit), "kernel"
    (the per-Gaussian kernel on incoming gradients) or "kernel+deposit" (both, added); None before the first.  Tests and tools."""
    return _last_path[0]


def _node_state(node):
    """(inputs, flags, wants, skinned, vertex gradient wanted) of a deform node, from what its forward saved."""
    lbs = isinstance(node, _LbsCageDeform._backward_cls)
    need = node.needs_input_grad
    inputs = _deform_saved(node.saved_tensors, node.has_dbary if lbs else node.has_delta)
    o = 6 if lbs else 0                     # _LbsCageDeform: lbs_cage's seven inputs stand where _CageDeform has tetpoints
    wants = dict(want_barys=need[o + 3] or need[o + 7], want_scales=need[o + 5], want_rotations=need[o + 6])
    return inputs, node.flags, wants, lbs, (True if lbs else need[0])


def claim_for_render(means3D, cov3D_precomp):
    """-> (node, token): the deform node that made both tensors, claimed for the calling render, or (None, None) -- the render
    then goes the usual way: fusion is on, gradients are recorded, the two tensors are outputs 0 and 1 of ONE _CageDeform /
    _LbsCageDeform node that no earlier render of this forward pass has claimed (a second one revokes the first one's claim), and
    nobody asked for their own gradients (retain_grad, tensor hooks).  The claim holds while `holds_claim(node, token)`: the
    token remembers the two tensors, and a retain_grad() or hook that arrives between the render and its backward ends the claim
    there (the render then returns their gradients as always)."""
    none = (None, None)
    if not _fusion["enabled"] or means3D is None or cov3D_precomp is None or not torch.is_grad_enabled():
        return none
    node = means3D.grad_fn
    if node is None or node is not cov3D_precomp.grad_fn or means3D.shape[0] == 0:
        return none
    if not isinstance(node, (_CageDeform._backward_cls, _LbsCageDeform._backward_cls)):
        return none
    if means3D.output_nr != 0 or cov3D_precomp.output_nr != 1:
        return none
    if getattr(node, "claimed", _REVOKED) is not False:
        node.claimed = _REVOKED
        return none
    if getattr(node.binding, "_render_fusion_demoted", None) == _fusion["epoch"]:
        return none
    if _wants_own_gradient(means3D, cov3D_precomp):
        return none
    token = _Claim(means3D, cov3D_precomp)
    node.claimed = token.key
    return node, token


class _Claim:
    """A render's claim: the key the node carries while it holds, and the two tensors (kept by the render alone -- the node must
    not reference its own outputs)."""

    def __init__(self, *tensors):
        self.key, self.tensors = object(), tensors


def _wants_own_gradient(*tensors):
    return any(t.retains_grad or t._backward_hooks for t in tensors)


def holds_claim(node, token):
    """Asked by the claimed render's backward: is the node still its own, and does still nobody want the two tensors' gradients?"""
    if node is None or token is None or getattr(node, "claimed", None) is not token.key:
        return False
    if _wants_own_gradient(*token.tensors):
        node.claimed = False
        return False
    return True


def release_claim(node, token):
    """A claimed render that cannot take the fused path after all (its operator found a reason) gives the node back."""
    if node is not None and token is not None and getattr(node, "claimed", None) is token.key:
        node.claimed = False


def fused_tail_structs(node):
    """For the claimed render's backward: (struct d3ga_cage_deform_in, struct d3ga_cage_deform_grads, struct d3ga_cage_deform_route
    | None, deposit) of `node` with fresh outputs.  The caller passes the three structs to a d3ga_raster_*_deform entry and then
    hands `deposit` (which keeps every tensor alive) to `deposit_on`."""
    inputs, flags, wants, skinned, want_v = _node_state(node)
    st = _deform_in(flags=flags, **inputs)
    P, V, dev = st.P, st.V, inputs["barys"].device
    new = lambda c, on: torch.empty((P, c), dtype=torch.float32, device=dev) if on else None
    g_b, g_s, g_r = new(4, wants["want_barys"]), new(3, wants["want_scales"]), new(4, wants["want_rotations"])
    grads = _lib.CageDeformGrads(g_means=None, g_cov6=None, g_tetpoints=None, g_barys=dptr(g_b), g_scales=dptr(g_s), g_rots=dptr(g_r))
    merged = _route_choice(P, want_v, skinned)
    route = records = None
    if merged is not None:
        route, records, merged = _route(inputs["tetras"], inputs["tetra_id"], P, V, dev, merged)
    return st, grads, route, dict(barys=g_b, scales=g_s, rotations=g_r, records=records, merged=merged, pins=inputs, binding=node.binding)


def deposit_on(node, deposit):
    node.deposit = deposit


def _take_deposit(ctx):
    """The node's deposit, if a claimed render left one; deposit and claim are cleared whatever happens next."""
    deposit, ctx.deposit, ctx.claimed = getattr(ctx, "deposit", None), None, False
    if deposit is not None:
        deposit.pop("pins", None)
    return deposit


class _CageDeform(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tetpoints, tetras, tetra_id, barys, canon_grad, scales, rotations, delta_barys, flags):
        require_cuda(tetpoints, tetras, tetra_id, barys, canon_grad, scales, rotations)
        tetpoints, barys, canon_grad, scales, rotations, delta_barys = map(
            _f32c, (tetpoints, barys, canon_grad, scales, rotations, delta_barys))
        ctx.flags = flags
        ctx.has_delta = delta_barys is not None
        ctx.claimed, ctx.deposit, ctx.binding = False, None, tetra_id          # render fusion (above)
        means, cov6 = _deform_fwd(_deform_in(tetpoints, tetras, tetra_id, barys, canon_grad, scales, rotations, delta_barys, flags),
                                  barys.device)
        ctx.set_materialize_grads(False)                 # backward() fills in the gradient of an unused output itself
        ctx.save_for_backward(tetpoints, tetras, tetra_id, barys, canon_grad, scales, rotations,
                              delta_barys if delta_barys is not None else torch.empty(0, device=barys.device))
        return means, cov6

    @staticmethod
    def backward(ctx, g_means, g_cov6):
        need = ctx.needs_input_grad
        deposit = _take_deposit(ctx)
        g = _deform_bwd(_deform_saved(ctx.saved_tensors, ctx.has_delta), ctx.flags, g_means, g_cov6, want_tetpoints=need[0],
                        want_barys=need[3] or need[7], want_scales=need[5], want_rotations=need[6], deposit=deposit)
        return (g["vertices"], None, None, g["barys"] if need[3] else None, None, g["scales"], g["rotations"],
                g["barys"] if need[7] else None, None)


def _deform_flags(op, barys, tetras, canonical_gradient, scale_activation, gradient_per_tet, say_which):
    """The argument checks cage_deform and lbs_cage_deform share -> the D3GA_DEFORM_* flags.  op: the caller's name, for its
    warning (raised at ITS caller: stacklevel 3); say_which: name the expected layout in the error."""
    if scale_activation not in (None, "exp"):
        raise ValueError(f"scale_activation must be None or 'exp', got {scale_activation!r}")
    P, T = barys.shape[0], tetras.shape[0]
    if gradient_per_tet is None:             # (T,3,3) is recognised by its length unless T == P (then say which)
        if canonical_gradient.shape[0] == T and T == P:
            warnings.warn(f"{op}: as many tetrahedra as Gaussians -- canonical_gradient is read per GAUSSIAN (the reference's "
                          "layout, lib/cage.py:329); pass gradient_per_tet=True if it is the per-tetrahedron table", stacklevel=3)
        gradient_per_tet = canonical_gradient.shape[0] == T and T != P
    if canonical_gradient.shape[0] != (T if gradient_per_tet else P):
        which = f" ({'one per tetrahedron' if gradient_per_tet else 'one per Gaussian'})" if say_which else ""
        raise ValueError(f"canonical_gradient has {canonical_gradient.shape[0]} matrices, expected {T if gradient_per_tet else P}{which}")
    return (1 if scale_activation == "exp" else 0) | (2 if gradient_per_tet else 0)


def cage_deform(tetpoints, tetras, tetra_id, barys, canonical_gradient, scales, rotations, delta_barys=None,
                scale_activation=None, gradient_per_tet=None):
    """(tetpoints (V,3), tetras (T,4), tetra_id (P), barys (P,4), canonical_gradient (P,3,3), scales (P,3),
    rotations (P,4) wxyz) -> (means3D (P,3), cov3D_precomp (P,6)); differentiable in tetpoints, barys, scales,
    rotations.  Drop-in for models/cage_net.py:218-230.  Index tensors may be int64
    (as the reference registers them, lib/cage.py:331-337); they are converted to int32 once per call --
    pass int32 to avoid the copy.

    Optional fusion of the two activations in front of the op (models/cage_net.py:213-214):
    `delta_barys` (P,4) is added to `barys` inside the kernel (differentiable), and `scale_activation="exp"` makes
    `scales` the raw log-scales (`scaling + delta`), with exp applied on load and the chain rule in the backward.

    `canonical_gradient` may also be ONE matrix per tetrahedron, (T,3,3) = `canonical_gradient_per_tet(...)` (round 4): the
    reference gathers the same matrices per Gaussian at init (lib/cage.py:329), which makes the op stream 36 B x P per pass;
    the per-tet table is read through `tetra_id` and stays in L2."""
    flags = _deform_flags("cage_deform", barys, tetras, canonical_gradient, scale_activation, gradient_per_tet, True)
    return _CageDeform.apply(tetpoints, _i32c(tetras), _i32c(tetra_id), barys, canonical_gradient, scales, rotations,
                             delta_barys, flags)


_POSE_CHUNK = 256         # = kBlock of csrc/deform.hip: the entries of one workgroup of the by-joint reduction


def lbs_pose_plan(skin_idx, J):
    """Static by-joint plan of the pose backward of lbs_cage / lbs_cage_deform (struct d3ga_lbs_pose_grad), built once per
    binding and cached by the storage of `skin_idx` (V,K) and J:
    -> dict(entries (V*K) int32 = the flat indices v*K + k sorted by joint (stable), chunk_range (n_chunks,2) int32 = [begin,
            end) of every chunk of at most 256 entries of one joint, chunk_ptr (J+1) int32 = the first chunk of each joint,
            n_chunks, n_entries, counter = the reduction's arrival count, kept at 0 between calls).
    The pelvis and spine joints of SMPL-X carry thousands of entries: they get many chunks (workgroups), summed in chunk order.
    Refuses (ValueError) an index outside [0, J) -- the forward would read outside joint_mats.  Building the plan reads two
    numbers back to the host; calls that hit the cache do not synchronise (capturable)."""
    if skin_idx.dim() != 2:
        raise ValueError(f"skin_idx must be (V,K), got {tuple(skin_idx.shape)}")
    if J <= 0:
        raise ValueError(f"joint_mats must hold at least one joint, got J = {J}")
    def build():
        with torch.no_grad():
            dev = skin_idx.device
            V, K = skin_idx.shape
            flat = skin_idx.reshape(-1).long()
            if flat.numel():
                bad = (flat < 0) | (flat >= J)
                nb = torch.nonzero(bad)
                if nb.numel():
                    q = int(nb[0, 0])
                    raise ValueError(f"skin_idx[{q // K}, {q % K}] = {int(flat[q])} is outside [0, {J}) (J = joint_mats.shape[0]; "
                                     f"{nb.shape[0]} such entries)")
            order = torch.sort(flat, stable=True)[1]
            counts = torch.bincount(flat, minlength=J)
            start = torch.zeros(J + 1, dtype=torch.int64, device=dev)
            start[1:] = torch.cumsum(counts, 0)
            nch = (counts + _POSE_CHUNK - 1) // _POSE_CHUNK
            chunk_ptr = torch.zeros(J + 1, dtype=torch.int64, device=dev)
            chunk_ptr[1:] = torch.cumsum(nch, 0)
            cj = torch.repeat_interleave(torch.arange(J, device=dev), nch)          # joint of every chunk
            q = torch.arange(cj.numel(), device=dev) - chunk_ptr[cj]
            beg = start[cj] + q * _POSE_CHUNK
            end = torch.minimum(beg + _POSE_CHUNK, start[cj + 1])
            return dict(entries=order.to(torch.int32).contiguous(), chunk_range=torch.stack([beg, end], 1).to(torch.int32).contiguous(),
                        chunk_ptr=chunk_ptr.to(torch.int32).contiguous(), n_chunks=int(cj.numel()), n_entries=V * K, J=J,
                        counter=torch.zeros(1, dtype=torch.int32, device=dev))
    return _pose_plan_cache.get((skin_idx,), J, build)


def sparse_skin_weights(dense_w, rows=None, K=None):
    """Exact K-sparse form of the dense skinning weights `dense_w[rows]` ((V,J) -> skin_idx (V,K) int32, skin_w (V,K)), the layout
    lbs_cage / lbs_cage_deform take.  The reference skins the cage with `skin_weights[nn_ids]` rows of a dense (V, 55) table
    (lib/smplman.py:155-164): pass that table and `rows=nn_ids`.  Each row keeps its non-zero weights in joint order; K is the
    largest non-zero count unless given (a K below it is refused), and shorter rows are padded with weight 0 (on joints whose
    weight is 0, or joint 0 beyond J).  Runs on whatever device the table lives."""
    if dense_w.dim() != 2:
        raise ValueError(f"dense_w must be (V,J), got {tuple(dense_w.shape)}")
    W = dense_w if rows is None else dense_w[rows.long() if torch.is_tensor(rows) else rows]
    V, J = W.shape
    nz = W != 0
    kmax = int(nz.sum(1).max()) if V else 0
    if K is None:
        K = max(kmax, 1)
    elif K < kmax:
        raise ValueError(f"K = {K} drops weights: a row has {kmax} non-zero entries")
    elif K < 1:
        raise ValueError(f"K must be >= 1, got {K}")
    order = torch.sort((~nz).to(torch.int8), dim=1, stable=True)[1]            # non-zero joints first, each group in joint order
    k = min(K, J)
    idx = order[:, :k]
    w = torch.gather(W, 1, idx)
    if K > J:
        idx = torch.cat([idx, idx.new_zeros(V, K - J)], 1)
        w = torch.cat([w, w.new_zeros(V, K - J)], 1)
    return idx.to(torch.int32).contiguous(), w.contiguous()


_POSE_INPUTS = (2, 5, 6)     # joint_mats, Rh, Th among the inputs of _LbsCage and _LbsCageDeform, which both start with lbs_cage's seven


def _check_pose_plan(skin_idx, joint_mats, Rh, Th):
    """With a pose gradient to come, build (or find) the by-joint plan now: it refuses an index outside [0, J) before the forward
    would read joint_mats through it."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (joint_mats, Rh, Th)):
        lbs_pose_plan(skin_idx, joint_mats.shape[0])


def _pose_grad_struct(plan, V, fused, template, delta, dev):
    """(struct, outputs, scratch) of one pose backward call; the tensors must stay alive until the launches are queued."""
    nbytes = ctypes.c_int64(0)
    check(_lib.lib().d3ga_lbs_pose_scratch_bytes(V, plan["n_chunks"], fused, ctypes.byref(nbytes)), "d3ga_lbs_pose_scratch_bytes")
    scratch = torch.empty((nbytes.value + 3) // 4, dtype=torch.float32, device=dev)
    J = plan["J"]
    gA = torch.empty((J, 4, 4), dtype=torch.float32, device=dev)
    gRh = torch.empty((3, 3), dtype=torch.float32, device=dev)
    gTh = torch.empty((3,), dtype=torch.float32, device=dev)
    st = _lib.LbsPoseGrad(J=J, n_chunks=plan["n_chunks"], n_entries=plan["n_entries"], tmpl=dptr(template), delta=dptr(delta),
                          chunk_ptr=dptr(plan["chunk_ptr"]), chunk_range=dptr(plan["chunk_range"]), entries=dptr(plan["entries"]),
                          counter=dptr(plan["counter"]), scratch=dptr(scratch), g_joint_mats=dptr(gA), g_Rh=dptr(gRh), g_Th=dptr(gTh))
    return st, (gA, gRh, gTh), scratch


def _pose_zeros(J, dev):
    """The pose gradients of a cage without vertices (the C ABI takes `pose` with V > 0 only)."""
    return torch.zeros((J, 4, 4), device=dev), torch.zeros((3, 3), device=dev), torch.zeros((3,), device=dev)


def _lbs_fwd(ctx, template, delta, joint_mats, skin_idx, skin_w, Rh, Th):
    """The skinning launch of both nodes and what their backward keeps of it
    -> (posed vertices (V,3), tensors to save: joint_mats, skin_idx, skin_w, Rh, then template, delta when a pose gradient is wanted)."""
    ctx.pose = any(ctx.needs_input_grad[i] for i in _POSE_INPUTS)
    if ctx.pose:
        ctx.shape_A, ctx.shape_Rh, ctx.shape_Th = (joint_mats.shape, None if Rh is None else Rh.shape,
                                                   None if Th is None else Th.shape)
    template, delta, joint_mats, skin_w, Rh, Th = map(_f32c, (template, delta, joint_mats, skin_w, Rh, Th))
    V, K = skin_w.shape
    out = torch.empty((V, 3), dtype=torch.float32, device=template.device)
    check(_lib.lib().d3ga_lbs_cage_fwd(V, K, dptr(template), dptr(delta), dptr(joint_mats), dptr(skin_idx),
                                       dptr(skin_w), dptr(Rh), dptr(Th), dptr(out), stream_handle()),
          "d3ga_lbs_cage_fwd")
    ctx.has_Rh, ctx.has_Th, ctx.has_delta = Rh is not None, Th is not None, delta is not None
    none = torch.empty(0, device=out.device)
    pose = (template, delta if delta is not None else none) if ctx.pose else ()     # the pose gradients read p~ = template + delta
    return out, (joint_mats, skin_idx, skin_w, Rh if Rh is not None else none) + pose


def _lbs_saved(ctx, saved):
    """What _lbs_fwd saved, by name -> dict(joint_mats, skin_idx, skin_w, Rh | None), and dict(template, delta | None) when this
    backward owes a pose gradient, else None."""
    skin = dict(zip(("joint_mats", "skin_idx", "skin_w", "Rh"), saved[:4]))
    if not ctx.has_Rh:
        skin["Rh"] = None
    pose = None
    if ctx.pose and any(ctx.needs_input_grad[i] for i in _POSE_INPUTS):
        pose = dict(template=saved[4], delta=saved[5] if ctx.has_delta else None)
    return skin, pose


def _lbs_returns(ctx, g_d, pose_out):
    """The gradients of lbs_cage's seven inputs from dL/d(delta) and the (gA, gRh, gTh) | None of the pose backward."""
    need = ctx.needs_input_grad
    gA, gRh, gTh = (None, None, None) if pose_out is None else (
        pose_out[0].view(ctx.shape_A) if need[2] else None, pose_out[1].view(ctx.shape_Rh) if (ctx.has_Rh and need[5]) else None,
        pose_out[2].view(ctx.shape_Th) if (ctx.has_Th and need[6]) else None)
    return g_d if need[0] else None, g_d if (ctx.has_delta and need[1]) else None, gA, None, None, gRh, gTh


class _LbsCage(torch.autograd.Function):
    @staticmethod
    def forward(ctx, template, delta, joint_mats, skin_idx, skin_w, Rh, Th):
        require_cuda(template, delta, joint_mats, skin_idx, skin_w, Rh, Th)
        out, saved = _lbs_fwd(ctx, template, delta, joint_mats, skin_idx, skin_w, Rh, Th)
        ctx.save_for_backward(*saved)
        return out

    @staticmethod
    def backward(ctx, g):
        skin, pose = _lbs_saved(ctx, ctx.saved_tensors)
        joint_mats, skin_idx, skin_w, Rh = skin["joint_mats"], skin["skin_idx"], skin["skin_w"], skin["Rh"]
        V, K = skin_w.shape
        J, dev, g = joint_mats.shape[0], g.device, _f32c(g)
        gd = torch.empty((V, 3), dtype=torch.float32, device=dev)
        st = pose_out = None
        if pose is not None and V == 0:
            pose_out = _pose_zeros(J, dev)
        else:
            if pose is not None:
                st, pose_out, scratch = _pose_grad_struct(lbs_pose_plan(skin_idx, J), V, 0, pose["template"], pose["delta"], dev)
            check(_lib.lib().d3ga_lbs_cage_bwd(V, K, dptr(joint_mats), dptr(skin_idx), dptr(skin_w), dptr(Rh), dptr(g), dptr(gd),
                                               None if st is None else ctypes.byref(st), stream_handle()), "d3ga_lbs_cage_bwd")
        return _lbs_returns(ctx, gd, pose_out)


def skeleton_matrices(bind_state, target_states):
    """(B,J,4,4) joint matrices for `lbs_cage` from Goliath-style skeleton states (translation 3 | quaternion xyzw 4 | scale 1):
    M_j = T_target,j . T_bind,j^-1 -- what lbsmodel/body_model.py:350-387 (states_to_matrix) hands to LinearBlendSkinning.skinning
    (:208-234), whose (V,8) skin_indices / skin_weights buffers are `lbs_cage`'s skin_idx / skin_w as they are.  A few dozen joints
    per pose: plain torch on whatever device the states live on.  bind_state (1,J,8) | (J,8), target_states (B,J,8) | (J,8)."""
    def split(s):
        return s[..., 0:3], s[..., 3:7] / s[..., 3:7].norm(dim=-1, keepdim=True), s[..., 7:8]

    def qmul(a, b):                                        # Hamilton product, xyzw
        av, aw, bv, bw = a[..., :3], a[..., 3:], b[..., :3], b[..., 3:]
        return torch.cat([aw * bv + bw * av + torch.cross(av, bv, dim=-1), aw * bw - (av * bv).sum(-1, keepdim=True)], -1)

    def qrot(q, v):
        qv, qw = q[..., :3], q[..., 3:]
        c = torch.cross(qv, v, dim=-1)
        return v + 2.0 * (qw * c + torch.cross(qv, c, dim=-1))
    bt, bq, bs = split(bind_state)
    tt, tq, ts = split(target_states)
    bq_inv = bq * bq.new_tensor([-1.0, -1.0, -1.0, 1.0])
    q = qmul(tq, bq_inv)                                   # rotation of the composed map
    sc = ts / bs                                           # its scale
    t = tt - sc * qrot(q, bt.expand_as(tt) if bt.dim() == tt.dim() else bt)      # x -> sc R(q) (x - t_bind) + t_target
    x, y, z, w = q.unbind(-1)
    R = torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     torch.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     torch.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)
    M = torch.zeros(q.shape[:-1] + (4, 4), dtype=q.dtype, device=q.device)
    M[..., :3, :3] = R * sc[..., None]
    M[..., :3, 3] = t
    M[..., 3, 3] = 1.0
    return M


def lbs_cage(template, delta, joint_mats, skin_idx, skin_w, Rh=None, Th=None):
    """K-sparse linear blend skinning of cage vertices: (sum_k w_k A[idx_k]) [v+delta;1], then .Rh^T + Th
    (lib/smplman.py:155-171).  Differentiable in template and delta (the deformation_field output when
    train.tet_offset_pre_lbs is on, models/cage_net.py:207-208), and in joint_mats (J,4,4), Rh (3,3) and Th (3,): the body pose
    reaches the cage through them (use_opt_smplx, models/garment_net.py:211-236).  dL/d(joint_mats) has an exact-zero bottom row
    (never read).  When one of the three requires a gradient, every skin_idx must lie in [0, J) (ValueError otherwise) and a
    by-joint plan is built once per binding (lbs_pose_plan); without pose gradients the backward is the one launch it always was."""
    skin_idx = _i32c(skin_idx)
    _check_pose_plan(skin_idx, joint_mats, Rh, Th)
    return _LbsCage.apply(template, delta, joint_mats, skin_idx, skin_w, Rh, Th)


class _LbsCageDeform(torch.autograd.Function):
    """lbs_cage + cage_deform as ONE autograd node (round 5): the forward is the two launches of the separate operators; the
    backward merges the corner gradients per workgroup (merge_plan) and forms dL/d(delta) in the vertex-gather launch
    (struct d3ga_cage_deform_skin) -- one launch instead of the gather + d3ga_lbs_cage_bwd; the pose gradients take one more."""

    @staticmethod
    def forward(ctx, template, delta, joint_mats, skin_idx, skin_w, Rh, Th, tetras, tetra_id, barys, canon_grad, scales, rotations,
                delta_barys, flags):
        require_cuda(template, delta, joint_mats, skin_idx, skin_w, Rh, Th, tetras, tetra_id, barys, canon_grad, scales, rotations)
        tetpoints, lbs_saved = _lbs_fwd(ctx, template, delta, joint_mats, skin_idx, skin_w, Rh, Th)
        barys, canon_grad, scales, rotations, delta_barys = map(_f32c, (barys, canon_grad, scales, rotations, delta_barys))
        ctx.flags, ctx.has_dbary = flags, delta_barys is not None
        ctx.claimed, ctx.deposit, ctx.binding = False, None, tetra_id          # render fusion (above)
        means, cov6 = _deform_fwd(_deform_in(tetpoints, tetras, tetra_id, barys, canon_grad, scales, rotations, delta_barys, flags),
                                  barys.device)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(tetpoints, tetras, tetra_id, barys, canon_grad, scales, rotations,
                              delta_barys if delta_barys is not None else torch.empty(0, device=barys.device), *lbs_saved)
        return means, cov6, tetpoints

    @staticmethod
    def backward(ctx, g_means, g_cov6, g_tp_extra):
        need = ctx.needs_input_grad
        deposit = _take_deposit(ctx)
        inputs = _deform_saved(ctx.saved_tensors, ctx.has_dbary)
        skin, pose = _lbs_saved(ctx, ctx.saved_tensors[8:])
        P, V, dev = inputs["barys"].shape[0], inputs["tetpoints"].shape[0], inputs["barys"].device
        want = dict(want_barys=need[9] or need[13], want_scales=need[11], want_rotations=need[12])
        if pose is not None and V == 0:                  # no cage: no Gaussian either
            zeros = lambda c, on: torch.zeros((P, c), device=dev) if on else None
            g = dict(vertices=torch.empty((0, 3), device=dev), pose=_pose_zeros(skin["joint_mats"].shape[0], dev),
                     barys=zeros(4, want["want_barys"]), scales=zeros(3, want["want_scales"]), rotations=zeros(4, want["want_rotations"]))
        else:
            g = _deform_bwd(inputs, ctx.flags, g_means, g_cov6, skin=dict(skin, g_extra=g_tp_extra), pose=pose, deposit=deposit, **want)
        return _lbs_returns(ctx, g["vertices"], g["pose"]) + (None, None, g["barys"] if need[9] else None, None, g["scales"],
                                                              g["rotations"], g["barys"] if need[13] else None, None)


def lbs_cage_deform(template, delta, joint_mats, skin_idx, skin_w, tetras, tetra_id, barys, canonical_gradient, scales, rotations,
                    delta_barys=None, scale_activation=None, gradient_per_tet=None, Rh=None, Th=None):
    """`cage_deform(lbs_cage(template, delta, joint_mats, skin_idx, skin_w, Rh, Th), tetras, ...)` as one operator (an extension
    like `renderer.render_l1`; lib/smplman.py:155-171 feeding models/cage_net.py:218-230): same outputs, same gradients, one
    launch less in the backward.  -> (means3D (P,3), cov3D_precomp (P,6), tetpoints (V,3)); the posed cage vertices are returned
    for the terms that read them directly (the FEM regulariser, lib/cage.py:349-361) -- their gradient joins the skinning backward.
    Differentiable in joint_mats, Rh and Th as lbs_cage is (the pose gradients take one launch more in the backward, and only
    when one of the three requires a gradient)."""
    flags = _deform_flags("lbs_cage_deform", barys, tetras, canonical_gradient, scale_activation, gradient_per_tet, False)
    skin_idx = _i32c(skin_idx)
    _check_pose_plan(skin_idx, joint_mats, Rh, Th)
    return _LbsCageDeform.apply(template, delta, joint_mats, skin_idx, skin_w, Rh, Th, _i32c(tetras), _i32c(tetra_id), barys,
                                canonical_gradient, scales, rotations, delta_barys, flags)


class _FemEnergy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tetpoints, tetras, Dn_inv):
        require_cuda(tetpoints, tetras, Dn_inv)
        tetpoints, Dn_inv = _f32c(tetpoints), _f32c(Dn_inv)
        T = tetras.shape[0]
        e = torch.empty((T,), dtype=torch.float32, device=tetpoints.device)
        check(_lib.lib().d3ga_fem_energy_fwd(T, dptr(tetpoints), dptr(tetras), dptr(Dn_inv), dptr(e), stream_handle()),
              "d3ga_fem_energy_fwd")
        ctx.save_for_backward(tetpoints, tetras, Dn_inv)
        return e

    @staticmethod
    def backward(ctx, g):
        tetpoints, tetras, Dn_inv = ctx.saved_tensors
        T, V = tetras.shape[0], tetpoints.shape[0]
        gt = torch.empty((V, 3), dtype=torch.float32, device=g.device)
        check(_lib.lib().d3ga_fem_energy_bwd(T, V, dptr(tetpoints), dptr(tetras), dptr(Dn_inv), dptr(_f32c(g)),
                                             dptr(gt), stream_handle()), "d3ga_fem_energy_bwd")
        return gt, None, None


def fem_energy(tetpoints, tetras, Dn_inv):
    """Per-tet 0.5 (det F - 1)^2 + 0.5 (tr F^T F - 3), F = Ds Dn^-1 (lib/cage.py:349-361).  Returns (T,)."""
    return _FemEnergy.apply(tetpoints, _i32c(tetras), Dn_inv)


def canonical_gradient(canon_points, tetras, tetra_id):
    """inv(Dm) per Gaussian (lib/cage.py:329); init-time, plain torch on whatever device the inputs live."""
    c = canon_points[tetras.long()][tetra_id.long()]
    Dm = torch.stack([c[:, 3] - c[:, 0], c[:, 2] - c[:, 0], c[:, 1] - c[:, 0]], dim=2)
    return torch.linalg.inv(Dm)


def canonical_gradient_per_tet(canon_points, tetras):
    """inv(Dm) per TETRAHEDRON, (T,3,3): `canonical_gradient(...)` == this[tetra_id]; accepted by cage_deform directly."""
    c = canon_points[tetras.long()]
    Dm = torch.stack([c[:, 3] - c[:, 0], c[:, 2] - c[:, 0], c[:, 1] - c[:, 0]], dim=2)
    return torch.linalg.inv(Dm)


def batch_rodrigues(rot_vecs, epsilon=1e-8):
    """Axis-angle vectors (B,3) -> rotation matrices (B,3,3): R = I + sin(t) K + (1 - cos(t)) K^2 with t = |r + eps|,
    K = [r / t]x.  This is the helper `tetra_sampler.lbs.batch_rodrigues` the reference imports at lib/smplman.py:16 and
    calls on the global rotation `Rh` (lib/smplman.py:167,203); tetra-sampler is un-vendored, so the published SMPL(-X)
    convention is restated here (parity unpinned; pinned by its group properties in tests/test_abi_and_host.py).  Needs no
    asset, runs on whatever device `rot_vecs` lives (init / per-pose glue, not a hot kernel)."""
    if rot_vecs.dim() != 2 or rot_vecs.shape[1] != 3:
        raise ValueError(f"batch_rodrigues expects (B,3) axis-angle vectors, got {tuple(rot_vecs.shape)}")
    angle = torch.linalg.norm(rot_vecs + epsilon, dim=1, keepdim=True)        # (B,1); eps keeps the zero rotation finite
    k = rot_vecs / angle
    s, c = torch.sin(angle)[:, :, None], torch.cos(angle)[:, :, None]
    z = torch.zeros_like(k[:, 0])
    K = torch.stack([z, -k[:, 2], k[:, 1], k[:, 2], z, -k[:, 0], -k[:, 1], k[:, 0], z], dim=1).view(-1, 3, 3)
    eye = torch.eye(3, dtype=rot_vecs.dtype, device=rot_vecs.device)[None]
    return eye + s * K + (1.0 - c) * torch.bmm(K, K)


# `tetra_sampler.body_model.SMPLlayer` (lib/smplman.py:9,68-74): the SMPL-X body model on the HIP kernels of
# csrc/body_model.hip.  Kept importable from here for callers of the earlier placeholder.
from .body_model import SMPLlayer  # noqa: E402,F401
