"""Barycentric attributes over cage and mesh bindings: the gather + `einsum("ikj,ik->ij", attr[cells][cell_id], barys)` of the
reference wherever it is applied to data other than the posed cage (include/d3ga.h D2b, csrc/bary_interp.hip):
    models/cage_net.py:236-241    -> cage_attr(pred_ao, tetras, tetra_id, barys, delta_bary, vertex_map=cage_to_body_vertex)
    models/cage_net.py:270        -> cage_attr(canon_tetpoints, tetras, tetra_id, barys)
    models/mesh_net.py:193,226    -> mesh_means(points, init_faces, init_barys, delta_bary)
The library sees a binding as ONE static table rows (P,K) -- corner k of Gaussian i reads row rows[i,k] of the attribute -- so one
kernel pair serves the three.  The backward into the attribute is a gather over the table's inverse (no float atomics, a fixed
order: bit-reproducible), the backward into the barycentrics one fma chain per Gaussian.  GPU tensors only for the op; the
binding's plan is plain torch and builds on whatever device its index tensors live.
"""
import torch

from . import _lib
from ._lib import D3GAError, check, dptr, f32c16, require_cuda, stream_handle
from .cage_deform import StorageCache, _f32c

_binding_cache = StorageCache()
MAX_C = 8                  # channels per row the kernels take (include/d3ga.h D2b)


def _in_range(ids, n, what):
    """Refuse (D3GAError) an id outside [0, n); reads one number back to the host."""
    if ids.numel() == 0:
        return
    lo, hi = int(ids.min()), int(ids.max())
    if lo < 0 or hi >= n:
        raise D3GAError(f"BaryBinding: {what} holds ids in [{lo}, {hi}], outside [0, {n})")


class BaryBinding:
    """Static description of who reads which row: built once, cached on its index tensors (as `vertex_adjacency` is).

        BaryBinding(rows, n_rows=V)                                      a (P,K) table as it is (the mesh binding: init_faces)
        BaryBinding(cells=tetras, cell_id=tetra_id, n_rows=V)            rows = cells[cell_id]   (the cage binding)
        ... vertex_map=cage_to_body_vertex                               rows = vertex_map[cells[cell_id]]; many-to-one is fine

    Holds `rows` (P,K) contiguous int32, `vert_start` (n_rows + 1) / `vert_items` (K P; item K i + k, stable by row) over the
    FINAL row ids -- so a gradient through a vertex map is summed per mapped row in a fixed order -- and `n_rows`, `K`, `P`.
    Every id is validated here, once (D3GAError otherwise; this reads numbers back to the host); the kernels check nothing and
    calls that hit the cache do not synchronise.  Works on CPU tensors too (the plan only)."""

    def __new__(cls, rows=None, *, cells=None, cell_id=None, vertex_map=None, n_rows):
        if (rows is None) == (cells is None) or (cells is None) != (cell_id is None):
            raise D3GAError("BaryBinding takes either a (P,K) table `rows` or `cells` (T,K) with `cell_id` (P,)")
        sources = tuple(t for t in (rows, cells, cell_id, vertex_map) if t is not None)
        for t in sources:
            if t.dtype not in (torch.int32, torch.int64):
                raise D3GAError(f"BaryBinding: index tensors are int32 or int64, got {t.dtype}")
        n_rows = int(n_rows)
        if n_rows < 0:
            raise D3GAError(f"BaryBinding: n_rows = {n_rows}")
        which = (rows is not None, vertex_map is not None, n_rows)
        return _binding_cache.get(sources, which, lambda: cls._build(rows, cells, cell_id, vertex_map, n_rows))

    @classmethod
    def _build(cls, rows, cells, cell_id, vertex_map, n_rows):
        with torch.no_grad():
            if rows is not None:
                if rows.dim() != 2:
                    raise D3GAError(f"BaryBinding: rows must be (P,K), got {tuple(rows.shape)}")
                final = rows.long()
            else:
                if cells.dim() != 2 or cell_id.dim() != 1:
                    raise D3GAError(f"BaryBinding: cells must be (T,K) and cell_id (P,), got {tuple(cells.shape)}, {tuple(cell_id.shape)}")
                _in_range(cell_id, cells.shape[0], "cell_id")
                final = cells.long()[cell_id.long()]
            K = final.shape[1]
            if K not in (3, 4):
                raise D3GAError(f"BaryBinding: K = {K} corners per Gaussian; the kernels take 3 (triangles) or 4 (tetrahedra)")
            if vertex_map is not None:
                if vertex_map.dim() != 1:
                    raise D3GAError(f"BaryBinding: vertex_map must be (Vcells,), got {tuple(vertex_map.shape)}")
                _in_range(final, vertex_map.shape[0], "cells[cell_id]" if rows is None else "rows")
                final = vertex_map.long()[final]
            _in_range(final, n_rows, "the final row table")
            P = final.shape[0]
            if K * P > 2**31 - 1:
                raise D3GAError(f"BaryBinding: {K} x {P} items do not fit int32")
            flat = final.reshape(-1)
            order = torch.sort(flat, stable=True)[1]
            start = torch.zeros(n_rows + 1, dtype=torch.int64, device=flat.device)
            start[1:] = torch.cumsum(torch.bincount(flat, minlength=n_rows), 0)
            self = object.__new__(cls)
            self.rows = _aligned16(final.to(torch.int32).contiguous())
            self.vert_start = start.to(torch.int32).contiguous()
            self.vert_items = order.to(torch.int32).contiguous()
            self.n_rows, self.K, self.P = n_rows, K, P
            return self


def _aligned16(t):
    """The K == 4 kernels read 16 bytes per Gaussian: a contiguous tensor whose storage offset breaks that is copied."""
    return t.clone() if t.data_ptr() % 16 else t


class _BaryInterp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, attr, barys, delta_barys, binding):
        require_cuda(attr, barys, delta_barys, binding.rows)
        P, K, V = binding.P, binding.K, binding.n_rows
        ctx.attr_shape = attr.shape
        attr2 = attr[:, None] if attr.dim() == 1 else attr
        if attr2.dim() != 2 or attr2.shape[0] != V or not 1 <= attr2.shape[1] <= MAX_C:
            raise D3GAError(f"bary_interp: attr must be ({V},C) or ({V},) with 1 <= C <= {MAX_C}, got {tuple(attr.shape)}")
        if tuple(barys.shape) != (P, K) or (delta_barys is not None and tuple(delta_barys.shape) != (P, K)):
            raise D3GAError(f"bary_interp: barys / delta_barys must be ({P},{K}), got {tuple(barys.shape)}"
                            + ("" if delta_barys is None else f" / {tuple(delta_barys.shape)}"))
        attr2, barys, delta_barys = _f32c(attr2), f32c16(barys), f32c16(delta_barys)
        C = attr2.shape[1]
        out = torch.empty((P, C), dtype=torch.float32, device=barys.device)
        check(_lib.lib().d3ga_bary_interp_fwd(P, K, C, dptr(attr2), dptr(binding.rows), dptr(barys), dptr(delta_barys), dptr(out),
                                              stream_handle()), "d3ga_bary_interp_fwd")
        ctx.binding, ctx.has_delta = binding, delta_barys is not None
        ctx.save_for_backward(attr2, barys, delta_barys if delta_barys is not None else torch.empty(0, device=barys.device))
        return out

    @staticmethod
    def backward(ctx, g_out):
        need_attr, need_barys = ctx.needs_input_grad[0], ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        attr2, barys, delta_barys = ctx.saved_tensors
        if not ctx.has_delta:
            delta_barys = None
        b = ctx.binding
        P, K, V, C, dev = b.P, b.K, b.n_rows, attr2.shape[1], barys.device
        g_attr = torch.empty((V, C), dtype=torch.float32, device=dev) if need_attr else None
        g_barys = torch.empty((P, K), dtype=torch.float32, device=dev) if need_barys else None
        check(_lib.lib().d3ga_bary_interp_bwd(P, V, K, C, dptr(attr2), dptr(b.rows), dptr(barys), dptr(delta_barys), dptr(_f32c(g_out)),
                                              dptr(b.vert_start), dptr(b.vert_items), dptr(g_attr), dptr(g_barys), stream_handle()),
              "d3ga_bary_interp_bwd")
        return (g_attr.view(ctx.attr_shape) if need_attr else None, g_barys if ctx.needs_input_grad[1] else None,
                g_barys if ctx.needs_input_grad[2] else None, None)


def bary_interp(attr, binding, barys, delta_barys=None):
    """out[i] = sum_k (barys + delta_barys)[i,k] attr[binding.rows[i,k]]: attr (V,C) or (V,) with C <= 8, barys and delta_barys
    (P,K) -> (P,C); the 1-D form returns (P,1), as the reference's `[..., None]` does.  Differentiable in attr, barys and
    delta_barys (the last two share one gradient); a gradient nobody needs is not formed, and without any there is no backward
    launch.  Inputs may be non-contiguous or of another float type (converted as the neighbouring ops do).  Bit-reproducible,
    never synchronises: capturable in `torch.cuda.graph` (build the binding before the capture)."""
    if not isinstance(binding, BaryBinding):
        raise D3GAError("bary_interp: binding must be a BaryBinding")
    return _BaryInterp.apply(attr, barys, delta_barys, binding)


def cage_attr(attr, tetras, tetra_id, barys, delta_barys=None, vertex_map=None):
    """A per-vertex attribute carried to the Gaussians of a cage binding.  Serves models/cage_net.py:236-241
    (`shadow = cage_attr(batch["pred_ao"], tetra_faces, tetra_id, geometry.barys, delta_bary, vertex_map=
    geometry.cage_to_body_vertex)`: attr is indexed by BODY vertex, its gradient is summed per body vertex) and
    models/cage_net.py:270 (`canonical_means3D = cage_attr(canon_tetpoints, tetra_faces, tetra_id, geometry.barys)`)."""
    return bary_interp(attr, BaryBinding(cells=tetras, cell_id=tetra_id, vertex_map=vertex_map, n_rows=attr.shape[0]), barys,
                       delta_barys)


def mesh_means(points, face_ids, barys, delta_barys=None):
    """The means of the mesh primitive: barycentric points on body-mesh triangles, `face_ids` (P,3) the three vertex ids stored
    per Gaussian.  Serves models/mesh_net.py:193 (`means3D`, with delta_barys = delta_bary) and :226 (`canonical_means3D`,
    without)."""
    return bary_interp(points, BaryBinding(face_ids, n_rows=points.shape[0]), barys, delta_barys)
