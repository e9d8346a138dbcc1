"""K nearest neighbours with distances and indices: pytorch3d's `knn_points` as the reference calls it
(models/cage_net.py:21,66: `knn_points(points[None], points[None], K = 4)[0][0, :, 1:].mean(-1)`), in HIP (csrc/knn.hip).
The semantics are stated in DESIGN.md 4.4j; they are this library's specification of record (pytorch3d cannot be run next to
it): float32 squared distances `dx*dx + dy*dy + dz*dz` (with the rounding of the three subtractions made up for, so that
they stay within 4 * 2^-24 d of the distance of the float32 coordinates wherever the query lies), neighbours ordered by
(distance, index) with the lower index first on equal distances, a query that is itself in `p2` finds itself, and `P2 < K`
pads the missing slots with dists = 0, idx = 0.

FORWARD ONLY: the reference calls it once, at construction, outside autograd; inputs that require grad are detached and the
results carry no graph (`knn`, the gathered neighbours of `return_nn=True`, is gathered from the detached `p2` as well).
GPU tensors only.  The exhaustive path never synchronises with the host; the grid path reads the bounding box of `p2` on the
host, once per batch element (an init-time call, like `tetra.knn_mean_dist2`).
"""
import ctypes
import math
from collections import namedtuple

import torch

from . import _lib
from ._lib import check, dptr, require_cuda, stream_handle
from .tetra import _grid_csr

_KNN = namedtuple("KNN", "dists idx knn")
MAX_K = 16               # D3GA_KNN_MAX_K (include/d3ga.h)
GRID_FROM = 2048         # method="auto": points of p2 per batch element from which the grid search is taken


def _full(lengths, N, P):
    if lengths is None:
        return True
    if torch.is_tensor(lengths):
        return lengths.numel() == N and bool((lengths.detach().cpu() == P).all())
    return False


def _grid(pts):
    """The uniform grid `tetra.knn_mean_dist2` buckets its points into (~4 per cell, at most ~256 cells per axis) ->
    (cell_start, cell_points, origin_h, dims) as d3ga_knn_points_grid takes them."""
    glo, ghi = pts.amin(0), pts.amax(0)
    box = torch.stack([glo, ghi]).cpu()                       # the one host read of this path
    if not bool(torch.isfinite(box).all()):
        raise ValueError("knn_points: p2 holds coordinates that are not finite")
    span = box[1] - box[0]
    P = pts.shape[0]
    vol = float(torch.clamp(span, min=1e-9).prod())
    h = max((vol / (P / 4.0)) ** (1.0 / 3.0), float(span.max()) / 256.0, 1e-12)
    dims = [max(1, int(math.ceil(float(span[a]) / h)) + 1) for a in range(3)]
    c = ((pts - glo) / h).floor().long()
    c = torch.minimum(c.clamp_min(0), torch.tensor([d - 1 for d in dims], device=pts.device))
    cell_start, cell_points = _grid_csr(c, c, dims)
    origin_h = (ctypes.c_float * 4)(float(box[0, 0]), float(box[0, 1]), float(box[0, 2]), h)
    return cell_start, cell_points, origin_h, (ctypes.c_int32 * 3)(*dims)


def knn_points(p1, p2, lengths1=None, lengths2=None, norm=2, K=1, version=-1, return_nn=False, return_sorted=True,
               method="auto"):
    """p1 (N,P1,3), p2 (N,P2,3) -> KNN(dists (N,P1,K) float32 squared distances ascending, idx (N,P1,K) int64 into p2,
    knn (N,P1,K,3) = p2[idx] if return_nn else None).  Forward only: inputs that require grad are detached.

    method: "exhaustive" (O(P1 P2), p2 streamed through LDS), "grid" (p2 bucketed into a uniform grid, exact ring search,
    one launch per batch element; bit-identical results) or "auto": the grid from 2048 points of p2 per element.
    `version` is accepted and ignored (pytorch3d's choice among its kernels).  Only what the reference uses is built: lengths
    other than None / full, norm != 2, D != 3 and return_sorted=False raise NotImplementedError; K > 16 raises ValueError."""
    what = "knn_points"
    if not torch.is_tensor(p1) or not torch.is_tensor(p2) or p1.dim() != 3 or p2.dim() != 3:
        raise ValueError(f"{what}: expected tensors p1 (N,P1,D) and p2 (N,P2,D)")
    if p1.shape[0] != p2.shape[0]:
        raise ValueError(f"{what}: p1 holds {p1.shape[0]} clouds, p2 {p2.shape[0]}")
    if p1.shape[2] != p2.shape[2]:
        raise ValueError(f"{what}: p1 has D = {p1.shape[2]}, p2 D = {p2.shape[2]}")
    if p1.shape[2] != 3:
        raise NotImplementedError(f"{what}: D = {p1.shape[2]}; only D = 3 is built")
    if norm != 2:
        raise NotImplementedError(f"{what}: norm = {norm!r}; only norm = 2 is built")
    if not return_sorted:
        raise NotImplementedError(f"{what}: return_sorted = False is not built (the result is always sorted)")
    N, P1, P2 = p1.shape[0], p1.shape[1], p2.shape[1]
    if not _full(lengths1, N, P1):
        raise NotImplementedError(f"{what}: lengths1 other than None or the full length is not built")
    if not _full(lengths2, N, P2):
        raise NotImplementedError(f"{what}: lengths2 other than None or the full length is not built")
    if isinstance(K, bool) or not isinstance(K, int) or K < 1:
        raise ValueError(f"{what}: K must be a positive integer, got {K!r}")
    if K > MAX_K:
        raise ValueError(f"{what}: K = {K} is more than the {MAX_K} this library keeps per query")
    if method not in ("auto", "grid", "exhaustive"):
        raise ValueError(f"{what}: method must be 'auto', 'grid' or 'exhaustive', got {method!r}")
    if N > 65535 or P2 >= 2 ** 31 - 1 or P1 >= 2 ** 31 - 1:
        raise ValueError(f"{what}: sizes ({N}, {P1}, {P2}) beyond what d3ga_knn_points accepts")
    require_cuda(p1, p2)
    a = p1.detach().float().contiguous()
    b = p2.detach().float().contiguous()
    dists = torch.empty((N, P1, K), dtype=torch.float32, device=a.device)
    idx = torch.empty((N, P1, K), dtype=torch.int64, device=a.device)
    L, s = _lib.lib(), stream_handle()
    grid = method == "grid" or (method == "auto" and P2 >= GRID_FROM)
    if grid and P2 > 0 and P1 > 0:
        for n in range(N):
            cell_start, cell_points, origin_h, dims = _grid(b[n])
            check(L.d3ga_knn_points_grid(P1, P2, K, dptr(a[n]), dptr(b[n]), dptr(cell_start), dptr(cell_points), origin_h, dims,
                                         dptr(dists[n]), dptr(idx[n]), s), "d3ga_knn_points_grid")
    else:
        check(L.d3ga_knn_points(N, P1, P2, K, dptr(a), dptr(b), dptr(dists), dptr(idx), s), "d3ga_knn_points")
    nn = None
    if return_nn:
        nn = torch.gather(b[:, None].expand(N, P1, P2, 3), 2, idx[..., None].expand(N, P1, K, 3)) if P2 > 0 else \
            torch.zeros((N, P1, K, 3), dtype=torch.float32, device=a.device)
    return _KNN(dists, idx, nn)
