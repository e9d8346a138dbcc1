"""Cage surface authoring (csrc/cage_author.hip): from the labelled star-pose body mesh to the closed surface that
TetGen fills -- with no trimesh, no mcubes, no open3d and no pass through the host.

    cager/ops.py:63-96    create_cage (scale, inflate, centre, voxelise, fill, isosurface)      prepare, voxelize, isosurface, create_cage
    cager/ops.py:38-60    smoothing(use_improved=True), 25 rounds                               smooth_improved, smooth_cage
    cager/ops.py:121-137  simplify: Taubin filter, winding, connected components                smooth_taubin, keep_components, simplify
    cager/ops.py:127-130  simplify_quadric_decimation (open3d)                                  decimate (csrc/decimate.hip)
    cager/ops.py:140-148  cage_processor                                                        cage_processor

The rules are pinned by csrc/cage_author_math.h, whose g++ build gives the kernels' bits.  Parity with trimesh's voxeliser, with
mcubes and with open3d is UNPINNED: none of them can run next to this library, so the specification of record is this one
(DESIGN.md 4.4u): the 13-axis triangle / closed-cube test in float64; `scipy.ndimage.binary_fill_holes` bit for bit; marching
TETRAHEDRA (six Kuhn tetrahedra per cell) on the grid padded with one empty layer, so the surface is always closed and a
2-manifold; Jacobi smoothers in float64 with one rounding to float32; parts labelled by their smallest face index.

Departures from the reference: quadric decimation runs only when asked for (`decimation="quadric"`; with the default None
`tris_target > 0` raises NotImplementedError) and is this library's rule -- rounds of independent collapses, csrc/decimate_math.h -- not
open3d's serial queue; `keep_components`
drops the vertices no kept face names (`drop_unreferenced=False` keeps them); a smoother never writes NaN -- a vertex without
faces or with a neighbour at distance 0 stays put and sets a status bit that `.check()` turns into ValueError; the winding repair
is one test of the signed volume (the isosurface is outward by construction).

Forward only, GPU tensors only.  This is set-up code: the fill reads one word back per round, the isosurface its two counts."""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import check, dptr, require_cuda, stream_handle
from .gauss_init import _as_tensor, _mesh
from .gauss_init import inflate as _inflate
from .template_bind import LoopPlan, _as_faces, _faces_i32, loop_plan

__all__ = ["VoxelGrid", "Smoothed", "prepare", "voxelize", "fill_holes", "isosurface", "smooth_improved", "smooth_taubin", "face_components",
           "keep_components", "create_cage", "smooth_cage", "simplify", "cage_processor", "Decimated", "decimate"]

_DECIMATION = "quadric decimation is not built yet; choose `radius` for the triangle count or decimate outside"


def _radius(what, radius):
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= int(radius) <= _lib.CAGE_MAX_RADIUS:
        raise ValueError(f"{what}: radius must be an integer in 1 .. {_lib.CAGE_MAX_RADIUS}, got {radius!r}")
    return int(radius)


def _number(what, name, x, positive=False):
    if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not math.isfinite(float(x)) or (positive and float(x) <= 0):
        raise ValueError(f"{what}: {name} must be a finite{' positive' if positive else ''} number, got {x!r}")
    return float(x)


def _count(what, name, x, lo, hi):
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not lo <= int(x) <= hi:
        raise ValueError(f"{what}: {name} must be an integer in {lo} .. {hi}, got {x!r}")
    return int(x)


def _split(what, vertices, faces):
    """(vertices, faces), or an object with .vertices and .faces in the place of both"""
    if faces is None:
        if not (hasattr(vertices, "vertices") and hasattr(vertices, "faces")):
            raise ValueError(f"{what}: give vertices and faces, or one object with .vertices and .faces")
        vertices, faces = vertices.vertices, vertices.faces
    return vertices, faces


def _checked_mesh(what, vertices, faces):
    v, f = _mesh(what, *_split(what, vertices, faces))
    if v.device.type != "meta" and not bool(torch.isfinite(v).all()):
        raise ValueError(f"{what}: vertices hold values that are not finite")
    return v, f


class VoxelGrid:
    """An occupancy grid of D = 2 radius + 1 voxels per axis with pitch = 1 / (radius + 0.1); voxel (i,j,k) is the closed cube centred
    at ((i,j,k) - radius) pitch.  `bits` (D, D, W) int64 on the device, indexed [z][y][x >> 6], bit x & 63.  `rounds`: the sweeps
    the fill took (None for a grid that was not filled)."""

    def __init__(self, radius, bits, rounds=None):
        self.radius = _radius("VoxelGrid", radius)
        self.D = 2 * self.radius + 1
        self.W = (self.D + 63) // 64
        if not torch.is_tensor(bits) or bits.dtype != torch.int64 or tuple(bits.shape) != (self.D, self.D, self.W) or not bits.is_contiguous():
            raise ValueError(f"VoxelGrid: bits must be a contiguous int64 tensor {(self.D, self.D, self.W)}")
        self.bits, self.rounds = bits, rounds

    @property
    def pitch(self):
        return 1.0 / (self.radius + 0.1)

    @classmethod
    def empty(cls, radius, device="cuda"):
        r = _radius("VoxelGrid.empty", radius)
        D = 2 * r + 1
        return cls(r, torch.zeros((D, D, (D + 63) // 64), dtype=torch.int64, device=device))

    @classmethod
    def from_dense(cls, dense, device=None):
        """dense (D,D,D) bool indexed [x,y,z], D odd -> VoxelGrid"""
        d = _as_tensor("VoxelGrid.from_dense", "dense", dense, device)
        if d.dim() != 3 or d.shape[0] != d.shape[1] or d.shape[0] != d.shape[2] or d.shape[0] % 2 == 0 or d.shape[0] < 3 or d.dtype != torch.bool:
            raise ValueError(f"VoxelGrid.from_dense: expected a bool array (D,D,D) with D odd and at least 3, got {tuple(d.shape)} {d.dtype}")
        D = d.shape[0]
        W = (D + 63) // 64
        zyx = torch.zeros((D, D, 64 * W), dtype=torch.int64, device=d.device)
        zyx[:, :, :D] = d.permute(2, 1, 0)
        shifts = torch.arange(64, dtype=torch.int64, device=d.device)
        return cls((D - 1) // 2, (zyx.reshape(D, D, W, 64) << shifts).sum(-1).contiguous())      # distinct bits: the sum is their OR

    def dense(self):
        """-> (D,D,D) bool, indexed [x,y,z]"""
        shifts = torch.arange(64, dtype=torch.int64, device=self.bits.device)
        zyx = ((self.bits[..., None] >> shifts) & 1).reshape(self.D, self.D, 64 * self.W)[:, :, :self.D]
        return zyx.permute(2, 1, 0).contiguous().bool()

    def desc(self, bits=None):
        return _lib.VoxelGridDesc(radius=self.radius, D=self.D, W=self.W, reserved=0, bits=(self.bits if bits is None else bits).data_ptr())


class Smoothed:
    """What a smoother returns: vertices (V,3) float32 and the sticky status word (1,) int32 on the device.  Unpacks as
    (vertices, status); `check()` reads the status back and raises ValueError for a vertex without faces or neighbours and for a
    zero-length edge."""

    def __init__(self, vertices, status):
        self.vertices, self.status = vertices, status

    def __iter__(self):
        return iter((self.vertices, self.status))

    def check(self):
        s = int(self.status.item())
        if s & _lib.CAGE_STATUS_RANGE:
            raise ValueError("smooth: an index outside its table")
        if s & _lib.CAGE_STATUS_ISOLATED:
            raise ValueError("smooth: a vertex has no face or no neighbour (the reference's weights would be NaN)")
        if s & _lib.CAGE_STATUS_ZERO_EDGE:
            raise ValueError("smooth: an edge has length 0 (the reference's weights would be infinite)")
        return self


def prepare(vertices, faces=None, inflate=0.01, scale=0.8):
    """The head of `create_cage`: x and y times `scale`, vertices moved by `inflate` along the angle-weighted normals of the scaled
    mesh (`gauss_init.inflate`), the vertex mean subtracted -> (vertices (V,3) float64, centre (3,) float64)."""
    what = "prepare"
    amount, scale = _number(what, "inflate", inflate), _number(what, "scale", scale, positive=True)
    v, f = _checked_mesh(what, vertices, faces)
    require_cuda(v, f)
    with torch.no_grad():
        v = v * torch.tensor([scale, scale, 1.0], dtype=torch.float64, device=v.device)
        v = _inflate(v, f, amount)
        centre = v.mean(0)
        return (v - centre).contiguous(), centre


def voxelize(vertices, faces=None, radius=60, fill=True):
    """`local_voxelize(mesh, [0,0,0], pitch, radius, fill)` by this library's rule -> VoxelGrid: a voxel is set iff a triangle meets
    its closed cube; geometry outside the grid is clipped.  fill=True also runs `fill_holes`."""
    what = "voxelize"
    r = _radius(what, radius)
    v, f = _checked_mesh(what, vertices, faces)
    require_cuda(v, f)
    grid = VoxelGrid.empty(r, v.device)
    status = torch.zeros(1, dtype=torch.int32, device=v.device)
    d = grid.desc()
    with torch.no_grad():
        check(_lib.lib().d3ga_cage_voxelize(ctypes.byref(d), v.shape[0], f.shape[0], dptr(v), dptr(f), dptr(status), stream_handle()), "d3ga_cage_voxelize")
    return fill_holes(grid) if fill else grid


def fill_holes(grid, check_every=1):
    """`scipy.ndimage.binary_fill_holes` of a grid, bit for bit -> a new VoxelGrid with `.rounds`: everything is occupied but the
    empty voxels 6-connected to the border through empty voxels.  `changed` is read back every `check_every` rounds."""
    what = "fill_holes"
    if not isinstance(grid, VoxelGrid):
        raise ValueError(f"{what}: grid must be a VoxelGrid, got {type(grid).__name__}")
    every = _count(what, "check_every", check_every, 1, 64)
    require_cuda(grid.bits)
    L, s, d = _lib.lib(), stream_handle(), grid.desc()
    outside, filled = torch.empty_like(grid.bits), torch.empty_like(grid.bits)
    changed = torch.zeros(1, dtype=torch.int32, device=grid.bits.device)
    rounds = 0
    with torch.no_grad():
        check(L.d3ga_cage_fill(ctypes.byref(d), _lib.CAGE_FILL_BEGIN, dptr(outside), None, None, s), "d3ga_cage_fill")
        while True:
            changed.zero_()
            for _ in range(every):
                check(L.d3ga_cage_fill(ctypes.byref(d), _lib.CAGE_FILL_ROUND, dptr(outside), None, dptr(changed), s), "d3ga_cage_fill")
            rounds += every
            if int(changed.item()) == 0:                     # the read-back
                break
        check(L.d3ga_cage_fill(ctypes.byref(d), _lib.CAGE_FILL_FINISH, dptr(outside), dptr(filled), None, s), "d3ga_cage_fill")
    return VoxelGrid(grid.radius, filled, rounds)


def isosurface(grid, centre=None, scale=None):
    """Marching tetrahedra of a VoxelGrid (padded with one empty layer) -> (vertices (n,3) float32, faces (m,3) int32), a closed
    2-manifold oriented outward.  Grid coordinate x becomes ((x / radius - 1) + centre) / scale; centre (3,) and scale (a number or
    (3,)) default to 0 and 1.  An empty grid gives (0,3) and (0,3)."""
    what = "isosurface"
    if not isinstance(grid, VoxelGrid):
        raise ValueError(f"{what}: grid must be a VoxelGrid, got {type(grid).__name__}")
    c = np.zeros(3) if centre is None else (centre.detach().cpu().numpy() if torch.is_tensor(centre) else np.asarray(centre)).astype(np.float64).reshape(-1)
    sc = np.ones(3) if scale is None else (scale.detach().cpu().numpy() if torch.is_tensor(scale) else np.asarray(scale, np.float64)).astype(np.float64).reshape(-1)
    sc = np.repeat(sc, 3) if sc.size == 1 else sc
    if c.shape != (3,) or sc.shape != (3,) or not np.isfinite(c).all() or not np.isfinite(sc).all() or (sc == 0).any():
        raise ValueError(f"{what}: centre must be three finite numbers and scale one or three that are not 0")
    require_cuda(grid.bits)
    dev = grid.bits.device
    L, s, d = _lib.lib(), stream_handle(), grid.desc()
    nbytes = ctypes.c_int64()
    check(L.d3ga_cage_iso_scratch_bytes(grid.radius, ctypes.byref(nbytes)), "d3ga_cage_iso_scratch_bytes")
    scratch = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    with torch.no_grad():
        check(L.d3ga_cage_iso_count(ctypes.byref(d), dptr(scratch), nbytes.value, dptr(counts), s), "d3ga_cage_iso_count")
        nv, nf = (int(x) for x in counts.cpu().tolist())     # the read-back
        vertices = torch.empty((nv, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((nf, 3), dtype=torch.int32, device=dev)
        if nv == 0 or nf == 0:
            return vertices, faces
        if 3 * max(nv, nf) > 2 ** 31 - 1:
            raise ValueError(f"{what}: {nv} vertices and {nf} faces: 3 n must stay below 2^31")
        out = _lib.CageIsoDesc(n_vertices=nv, n_faces=nf, centre=(ctypes.c_double * 3)(*c), scale=(ctypes.c_double * 3)(*sc),
                               vertices=vertices.data_ptr(), faces=faces.data_ptr())
        check(L.d3ga_cage_iso_emit(ctypes.byref(d), ctypes.byref(out), dptr(scratch), nbytes.value, s), "d3ga_cage_iso_emit")
    return vertices, faces


def _plan_type(what, plan):
    if plan is not None and not isinstance(plan, LoopPlan):
        raise ValueError(f"{what}: plan must be a LoopPlan, got {type(plan).__name__}")


def _plan_for(what, plan, f, V):
    if plan is None:
        plan = loop_plan(f, V)
    elif plan.V != V or plan.F != f.shape[0]:
        raise ValueError(f"{what}: the plan is of a mesh with V = {plan.V}, F = {plan.F}; this one has V = {V}, F = {f.shape[0]}")
    plan.check()
    if plan.E < 1:
        raise ValueError(f"{what}: the mesh has no edge")
    return plan


def _vertex_faces(plan):
    """vertex -> incident faces, ascending, as (offsets (V+1), faces) int32 on the device; kept on the plan"""
    if getattr(plan, "_vertex_faces", None) is None:
        flat = plan.faces.reshape(-1).long()
        order = torch.sort(flat, stable=True).indices          # stable: the faces of a vertex stay ascending
        offsets = torch.zeros(plan.V + 1, dtype=torch.int32, device=flat.device)
        offsets[1:] = torch.cumsum(torch.bincount(flat, minlength=plan.V), 0).to(torch.int32)
        plan._vertex_faces = (offsets, (order // 3).to(torch.int32).contiguous())
    return plan._vertex_faces


def _smooth(what, mode, vertices, faces, iterations, lam, mu, plan):
    iterations = _count(what, "the number of iterations", iterations, 1, _lib.CAGE_MAX_ITERATIONS)
    lam, mu = _number(what, "the step", lam), _number(what, "mu", mu)
    v, f = _checked_mesh(what, vertices, faces)
    _plan_type(what, plan)
    require_cuda(v, f)
    plan = _plan_for(what, plan, f, v.shape[0])
    dev, V = v.device, v.shape[0]
    x = v.clone()                                            # overwritten by the iterations
    work, out = torch.empty_like(x), torch.empty((V, 3), dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    d = _lib.CageSmoothDesc(mode=mode, iterations=iterations, lam=lam, mu=mu, x=x.data_ptr(), work=work.data_ptr(), out=out.data_ptr(),
                            status=status.data_ptr())
    if mode == _lib.CAGE_SMOOTH_IMPROVED:
        offsets, idx = _vertex_faces(plan)
        normals = torch.empty_like(x)
        d.normals, d.faces, d.csr_offsets, d.csr_faces = normals.data_ptr(), plan.faces.data_ptr(), offsets.data_ptr(), idx.data_ptr()
    st = plan.struct()
    with torch.no_grad():
        check(_lib.lib().d3ga_cage_smooth(ctypes.byref(st), ctypes.byref(d), stream_handle()), "d3ga_cage_smooth")
    return Smoothed(out, status)


def smooth_improved(vertices, faces=None, num_iter=25, lbd=0.25, plan=None):
    """`smoothing(mesh, num_iter, lbd, use_improved=True)` -> Smoothed(vertices (V,3) f32, status): num_iter Jacobi iterations of the
    normal-aware Laplacian in float64.  plan: the `template_bind.loop_plan(faces, V)` of this mesh (built here if None)."""
    return _smooth("smooth_improved", _lib.CAGE_SMOOTH_IMPROVED, vertices, faces, num_iter, lbd, 0.0, plan)


def smooth_taubin(vertices, faces=None, iterations=10, lam=0.5, mu=-0.53, plan=None):
    """open3d's `filter_smooth_taubin` -> Smoothed: per iteration v += lam (mean of the neighbours - v), then the same with mu."""
    return _smooth("smooth_taubin", _lib.CAGE_SMOOTH_TAUBIN, vertices, faces, iterations, lam, mu, plan)


def face_components(faces, n_vertices, plan=None):
    """-> (F,) int32: for every face the smallest face index of its part (faces that share an edge are adjacent)."""
    what = "face_components"
    if isinstance(n_vertices, bool) or not isinstance(n_vertices, (int, np.integer)) or not 1 <= int(n_vertices) <= (2 ** 31 - 1) // 3:
        raise ValueError(f"{what}: n_vertices must be an integer in 1 .. (2^31 - 1) / 3, got {n_vertices!r}")
    f = _faces_i32(_as_faces(what, faces))
    _plan_type(what, plan)
    require_cuda(f)
    plan = _plan_for(what, plan, f, int(n_vertices))
    L, s, st = _lib.lib(), stream_handle(), plan.struct()
    label = torch.empty(plan.F, dtype=torch.int32, device=f.device)
    changed = torch.zeros(1, dtype=torch.int32, device=f.device)
    with torch.no_grad():
        check(L.d3ga_cage_components(ctypes.byref(st), _lib.CAGE_PARTS_BEGIN, dptr(label), None, s), "d3ga_cage_components")
        while True:
            changed.zero_()
            check(L.d3ga_cage_components(ctypes.byref(st), _lib.CAGE_PARTS_ROUND, dptr(label), dptr(changed), s), "d3ga_cage_components")
            if int(changed.item()) == 0:                     # the read-back
                break
    return label


def keep_components(vertices, faces=None, min_faces=70, drop_unreferenced=True, plan=None):
    """The tail of `simplify`: parts of fewer than `min_faces` faces are dropped (faces compacted in order), vertices no kept face
    names are removed in ascending order (drop_unreferenced=False keeps them), and if the signed volume is negative every face
    is flipped -> (vertices (V',3), faces (F',3) int32).  Vertices keep their dtype."""
    what = "keep_components"
    min_faces = _count(what, "min_faces", min_faces, 0, 2 ** 31 - 1)
    vertices, faces = _split(what, vertices, faces)
    v, f = _checked_mesh(what, vertices, faces)
    keep_dtype = vertices.dtype if torch.is_tensor(vertices) else (torch.float32 if np.asarray(vertices).dtype == np.float32 else torch.float64)
    label = face_components(f, v.shape[0], plan)
    with torch.no_grad():
        sizes = torch.bincount(label.long(), minlength=f.shape[0])
        f = f[sizes[label.long()] >= min_faces]
        if f.shape[0]:
            a, b, c = (v[f[:, k].long()] for k in range(3))
            if float((a * torch.linalg.cross(b, c)).sum()) < 0:          # six times the signed volume
                f = f[:, [0, 2, 1]]
        if drop_unreferenced:
            used = torch.zeros(v.shape[0], dtype=torch.bool, device=v.device)
            used[f.reshape(-1).long()] = True
            renumber = torch.cumsum(used, 0) - 1
            v, f = v[used], renumber[f.long()].to(torch.int32)
    return v.to(keep_dtype).contiguous(), f.contiguous()


def create_cage(vertices, faces=None, radius=60, inflate=0.01, scale=0.8):
    """cager/ops.py::create_cage -> (vertices (n,3) float32, faces (m,3) int32): the isosurface of the filled voxelisation of the
    scaled, inflated, centred mesh, mapped back (`v / radius - 1`, + centre, x and y / scale)."""
    radius = _radius("create_cage", radius)
    v, centre = prepare(vertices, faces, inflate, scale)
    f = _split("create_cage", vertices, faces)[1]
    grid = voxelize(v, f, radius, fill=True)
    return isosurface(grid, centre=centre, scale=(float(scale), float(scale), 1.0))


def smooth_cage(vertices, faces=None, num_iter=25, lbd=0.25):
    """cager/ops.py::smooth_cage -> (vertices (V,3) float32, faces): `smooth_improved`, checked."""
    vertices, faces = _split("smooth_cage", vertices, faces)
    return smooth_improved(vertices, faces, num_iter, lbd).check().vertices, faces


class Decimated:
    """What `decimate` returns: vertices (V',3) float32, faces (F',3) int32, the sticky status word (1,) int32 on the device and the
    number of rounds run.  Unpacks as (vertices, faces); `check()` reads the status back and raises ValueError when the decimation
    ended above its target."""

    def __init__(self, vertices, faces, status, rounds, target):
        self.vertices, self.faces, self.status, self.rounds, self.target = vertices, faces, status, rounds, target

    def __iter__(self):
        return iter((self.vertices, self.faces))

    def check(self):
        s = int(self.status.item())
        if s & _lib.CAGE_STATUS_RANGE:
            raise ValueError("decimate: an index outside its table")
        if s & _lib.CAGE_STATUS_STUCK:
            raise ValueError(f"decimate: stopped at {self.faces.shape[0]} faces after {self.rounds} rounds, the target was {self.target}: no edge "
                             f"may collapse any more (boundaries are fixed, the link condition, flipped faces) or max_rounds is too small")
        return self


def decimate(vertices, faces=None, tris_target=None, max_rounds=None):
    """Quadric-error-metric edge-collapse decimation down to `tris_target` triangles (the place of open3d's
    `simplify_quadric_decimation`) -> Decimated(vertices (V',3) float32, faces (F',3) int32, status, rounds).  Rounds of independent
    collapses by the rules of csrc/decimate_math.h: per round the `loop_plan` of the current faces, a key per edge, one `torch.sort`,
    the ceil((F - target) / 2) cheapest edges admitted, an independent set of them collapsed, the faces compacted; two counts are
    read back.  A closed 2-manifold stays one, with its Euler characteristic and its parts; F' is the target or one less.  Boundary
    vertices never move.  tris_target >= F returns the input (without the vertices no face names) in zero rounds.  A round without
    a valid edge, or `max_rounds` (default CAGE_MAX_ITERATIONS) reached, sets the STUCK bit: the mesh as it stands is returned and
    `.check()` raises.  A mesh with an edge in three faces raises `LoopPlan.check()`'s ValueError."""
    what = "decimate"
    if tris_target is None:
        raise ValueError(f"{what}: tris_target is required")
    target = _count(what, "tris_target", tris_target, 1, 2 ** 31 - 1)
    max_rounds = _count(what, "max_rounds", _lib.CAGE_MAX_ITERATIONS if max_rounds is None else max_rounds, 1, _lib.CAGE_MAX_ITERATIONS)
    v, f = _checked_mesh(what, vertices, faces)
    require_cuda(v, f)
    dev, V = v.device, v.shape[0]
    L, s = _lib.lib(), stream_handle()
    x = v.clone()                                            # overwritten by the collapses
    quadrics = torch.empty((V, 10), dtype=torch.float64, device=dev)
    owner = torch.empty(V, dtype=torch.int64, device=dev)
    remap = torch.empty(V, dtype=torch.int32, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    nbytes = ctypes.c_int64()
    check(L.d3ga_decimate_scratch_bytes(f.shape[0], ctypes.byref(nbytes)), "d3ga_decimate_scratch_bytes")
    scratch = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    d = _lib.DecimateDesc(x=x.data_ptr(), quadrics=quadrics.data_ptr(), owner=owner.data_ptr(), remap=remap.data_ptr(), scratch=scratch.data_ptr(),
                          scratch_bytes=nbytes.value, counts=counts.data_ptr(), status=status.data_ptr())
    rounds = 0
    with torch.no_grad():
        while True:
            F = f.shape[0]
            need = (F - target + 1) // 2
            if need <= 0:
                break
            if rounds >= max_rounds:
                status |= _lib.CAGE_STATUS_STUCK
                break
            plan = _plan_for(what, None, f, V)
            offsets, idx = _vertex_faces(plan)
            st = plan.struct()
            keys = torch.empty(plan.E, dtype=torch.int64, device=dev)
            placement = torch.empty((plan.E, 3), dtype=torch.float64, device=dev)
            f_next = torch.empty_like(f)
            d.faces, d.csr_offsets, d.csr_faces, d.keys, d.placement, d.faces_out = (t.data_ptr() for t in (f, offsets, idx, keys, placement, f_next))
            if rounds == 0:
                check(L.d3ga_decimate_quadrics(ctypes.byref(st), ctypes.byref(d), s), "d3ga_decimate_quadrics")
            check(L.d3ga_decimate_candidates(ctypes.byref(st), ctypes.byref(d), s), "d3ga_decimate_candidates")
            sorted_keys = torch.sort(keys).values             # the keys are distinct: every one carries its edge
            d.sorted_keys, d.n_admit = sorted_keys.data_ptr(), min(need, plan.E)
            check(L.d3ga_decimate_collapse(ctypes.byref(st), ctypes.byref(d), s), "d3ga_decimate_collapse")
            check(L.d3ga_decimate_faces(ctypes.byref(st), ctypes.byref(d), s), "d3ga_decimate_faces")
            rounds += 1
            kept, valid = (int(c) for c in counts.cpu().tolist())           # the read-back
            if valid == 0:
                status |= _lib.CAGE_STATUS_STUCK
                break
            f = f_next[:kept]
        used = torch.zeros(V, dtype=torch.bool, device=dev)
        used[f.reshape(-1).long()] = True
        renumber = torch.cumsum(used, 0) - 1
        out_v, out_f = x[used].to(torch.float32).contiguous(), renumber[f.long()].to(torch.int32).contiguous()
    return Decimated(out_v, out_f, status, rounds, target)


def _decimation(what, decimation, tris_target):
    """-> whether to decimate; keeps the refusal of a positive target unless quadric decimation is asked for"""
    if decimation is not None and decimation != "quadric":
        raise ValueError(f"{what}: decimation must be None or 'quadric', got {decimation!r}")
    if tris_target > 0 and decimation is None:
        raise NotImplementedError(_DECIMATION)
    return tris_target > 0


def simplify(vertices, faces=None, tris_target=0, decimation=None):
    """cager/ops.py::simplify -> (vertices, faces): the Taubin filter, with decimation="quadric" and tris_target > 0 `decimate` down to
    tris_target, then winding and `keep_components(min_faces=70)`.  tris_target > 0 with decimation=None raises NotImplementedError."""
    tris_target = _count("simplify", "tris_target", tris_target, 0, 2 ** 31 - 1)
    reduce = _decimation("simplify", decimation, tris_target)
    vertices, faces = _split("simplify", vertices, faces)
    v = smooth_taubin(vertices, faces, iterations=10).check().vertices
    if reduce:
        v, faces = decimate(v, faces, tris_target).check()
    return keep_components(v, faces, min_faces=70)


def cage_processor(vertices, faces=None, cage_tris_target=0, radius=60, inflate=0.01, decimation=None):
    """cager/ops.py::cage_processor -> (vertices (1,V,3) float32, faces (1,F,3) int64), as the reference returns them.
    cage_tris_target > 0 needs decimation="quadric" (`simplify`)."""
    target = _count("cage_processor", "cage_tris_target", cage_tris_target, 0, 2 ** 31 - 1)
    _decimation("cage_processor", decimation, target)
    v, f = create_cage(vertices, faces, radius, inflate)
    if f.shape[0] == 0:
        raise ValueError("cage_processor: the voxelisation is empty: the mesh lies outside the grid")
    v, f = smooth_cage(v, f)
    v, f = simplify(v, f, target, decimation)
    return v.float()[None], f.long()[None]
