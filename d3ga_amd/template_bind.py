"""Template binding (csrc/template_bind.hip): what the reference's constructors leave on `self` between a body
model and the tensors the cage operators take -- with no trimesh, no kd-tree and no pass through the host.

    utils/mesh_utils.py:105-325   subdivide_loop (positions and the dense skinning table)      loop_plan, loop_subdivide
    lib/smplman.py:116-120        Smplman.find_nn (inflated template, nearest vertex)           nearest_vertex
    lib/smplman.py:55-59          Smplman.unpose (inverse of the blended transform)             unpose
    lib/smplman.py:122-143        get_star_pose                                                 star_pose
    lib/smplman.py:67-110         Smplman.create_body_model                                     bind_body_template
    lib/cage_smplman.py:54-76     CageSmpl.create_cage_model                                    bind_cage
    lib/cage_blueman.py:102-107   create_cage_skin_weights (Goliath)                            bind_cage_skin

The rules are pinned by csrc/template_bind_math.h, whose g++ build gives the kernels' bits: float64 arithmetic on float32 or float64
inputs, one rounding to float32 per output element, every sum in a fixed order, no float atomics.  Results depend on neither launch
geometry nor scheduling.

Specification of record (parity with trimesh is unpinned -- it cannot be run next to this):
  * unique edges are numbered in ascending order of (larger endpoint, smaller endpoint); row V + e is the odd vertex of edge e;
  * the boundary quirk: an even BOUNDARY vertex becomes (sum of the neighbours that are boundary vertices) / 8 + 0.75 v, and every
    such neighbour counts, also one reached across an interior edge (on the two-triangle quad the diagonal's ends have three);
  * nearest_vertex is `knn_points(K=1)`: float32 squared distances, ties to the lowest index; parity with a float64 kd-tree on
    near-ties is unpinned.
Three departures from the reference:
  * an edge in three or more faces sets a sticky status bit and `LoopPlan.check()` / `loop_subdivide` raise
    ValueError("... shared by more than 2 faces") (the reference enters a branch that calls `_subdivide` with two arguments);
  * a vertex that no face references keeps its position and attributes (the reference gives NaN: beta divides by k = 0);
  * a face index outside [0, V) sets a status bit (ValueError); so does a face that names one vertex twice.

Forward only, no gradient.  GPU tensors only.  One read-back per level of subdivision (number of edges, largest valence, status
word) and one per float input that is tested for values that are not finite: this is set-up code."""
import ctypes
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._lib import D3GAError, check, dptr, require_cuda, stream_handle

__all__ = ["LoopPlan", "loop_plan", "loop_subdivide", "beta_table", "nearest_vertex", "Unposed", "unpose", "star_pose", "TemplateBinding",
           "bind_body_template", "CageBinding", "bind_cage", "bind_cage_skin"]

TemplateBinding = namedtuple("TemplateBinding", "body_template_vertices body_template_faces skin_weights nn_ids")
CageBinding = namedtuple("CageBinding", "body_template_vertices nn_ids skin_idx skin_w")


def beta_table(max_valence):
    """beta_k = (40 - (2 cos(2 pi / k) + 3)^2) / (64 k) for k = 1 .. max_valence as float64, entry 0 unused (0): the table the
    even-vertex rule reads, built on the host so that kernel, g++ build and oracle share its bits."""
    k = np.arange(1, int(max_valence) + 1, dtype=np.float64)
    out = np.zeros(int(max_valence) + 1, np.float64)
    out[1:] = (40.0 - (2.0 * np.cos(2 * np.pi / k) + 3) ** 2) / (64 * k)
    return out


def _status_error(what, status):
    if status & _lib.BIND_STATUS_RANGE:
        return ValueError(f"{what}: an index outside its table (a face names a vertex outside [0, V), or a row / joint outside the skin table)")
    if status & _lib.BIND_STATUS_DEGENERATE:
        return ValueError(f"{what}: a face names one vertex twice")
    if status & _lib.BIND_STATUS_NONMANIFOLD:
        return ValueError(f"{what}: some edges are shared by more than 2 faces")
    if status & _lib.BIND_STATUS_SINGULAR:
        return ValueError(f"{what}: a blended transform is singular (|det| or the sum of the weights below 1e-12): nothing to invert")
    return None


class LoopPlan:
    """The topology of one level of Loop subdivision, on the device (int32 unless noted):
    edge_verts (E,2) smaller, larger endpoint -- edges in ascending (larger, smaller) order; edge_faces (E,2) the face of lower index
    and the other one or -1; edge_opp (E,2) their opposite vertices; edge_boundary (E) uint8; face_edge (F,3) face edge c = (corner c,
    corner c + 1) -> unique edge; vert_offsets (V+1), vert_nbr (2E) the neighbours of each vertex ascending; vert_boundary (V) uint8;
    `faces` (F,3) the faces it was built from.  V, F, E, max_valence and status are host integers (the one read-back)."""

    def __init__(self, faces, V, E, max_valence, status, tables, info):
        self.faces, self.V, self.F, self.E, self.max_valence, self.status = faces, V, faces.shape[0], E, max_valence, status
        self._full, self.info = tables, info
        t = tables
        self.edge_verts, self.edge_opp, self.edge_faces = t["edge_verts"][:E], t["edge_opp"][:E], t["edge_faces"][:E]
        self.edge_boundary, self.face_edge = t["edge_boundary"][:E], t["face_edge"]
        self.vert_offsets, self.vert_nbr, self.vert_boundary = t["vert_offsets"], t["vert_nbr"][:2 * E], t["vert_boundary"]
        self._beta = None

    @property
    def valence(self):
        return self.vert_offsets[1:] - self.vert_offsets[:-1]

    def beta(self):
        if self._beta is None:
            self._beta = torch.from_numpy(beta_table(max(self.max_valence, 1))).to(self.faces.device)
        return self._beta

    def struct(self, built=True):
        s = _lib.LoopPlanTables(V=self.V, F=self.F, E=self.E if built else 0, reserved=0)
        for k, t in self._full.items():
            setattr(s, k, t.data_ptr())
        return s

    def check(self):
        """Raises ValueError for the status the build read back: an edge in three or more faces, a face index outside [0, V), a
        face that names one vertex twice."""
        err = _status_error("loop_plan", self.status)
        if err is not None:
            raise err
        return self


def _as_faces(what, faces, device=None):
    if isinstance(faces, np.ndarray):
        if not torch.cuda.is_available():
            raise D3GAError("d3ga_amd ops run on the GPU only and no GPU is available; there is no CPU fallback")
        faces = torch.from_numpy(np.ascontiguousarray(faces)).to(device or "cuda")
    if not torch.is_tensor(faces):
        raise ValueError(f"{what}: faces must be a tensor or an array, got {type(faces).__name__}")
    faces = faces.detach()
    if faces.dim() == 3 and faces.shape[0] == 1:
        faces = faces[0]
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
        raise ValueError(f"{what}: expected faces (F,3) with F >= 1, got {tuple(faces.shape)}")
    if faces.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{what}: faces must be int32 or int64, got {faces.dtype}")
    if 6 * faces.shape[0] > 2 ** 31 - 1:
        raise ValueError(f"{what}: 6 F must stay below 2^31, got F = {faces.shape[0]}")
    return faces


def _faces_i32(faces):
    if faces.dtype == torch.int64:
        faces = faces.clamp(-1, 2 ** 31 - 1)                 # whatever lay outside int32 stays outside [0, V)
    return faces.to(torch.int32).contiguous()


def loop_plan(faces, n_vertices):
    """faces (F,3) int32 or int64 on the GPU, n_vertices = V -> LoopPlan.  The 64-bit keys are sorted by `torch.sort` (stable); runs,
    pairing, opposite vertices, counting, the scans and the neighbour lists are HIP.  One read-back.  Does not raise for a mesh
    it flags: `.check()` does (and `loop_subdivide` calls it)."""
    what = "loop_plan"
    faces = _as_faces(what, faces)
    if isinstance(n_vertices, bool) or not isinstance(n_vertices, (int, np.integer)) or not 1 <= int(n_vertices) <= 2 ** 31 - 1:
        raise ValueError(f"{what}: n_vertices must be an integer in 1 .. 2^31 - 1, got {n_vertices!r}")
    V, F = int(n_vertices), faces.shape[0]
    require_cuda(faces)
    dev = faces.device
    f32 = _faces_i32(faces)
    L, s = _lib.lib(), stream_handle()
    i32 = dict(dtype=torch.int32, device=dev)
    info = torch.zeros(4, **i32)
    status = info[2:3]
    keys = torch.empty(3 * F, dtype=torch.int64, device=dev)
    tables = {"edge_verts": torch.empty((3 * F, 2), **i32), "edge_opp": torch.empty((3 * F, 2), **i32),
              "edge_faces": torch.empty((3 * F, 2), **i32), "edge_boundary": torch.empty(3 * F, dtype=torch.uint8, device=dev),
              "face_edge": torch.empty((F, 3), **i32), "vert_offsets": torch.empty(V + 1, **i32), "vert_nbr": torch.empty(6 * F, **i32),
              "vert_boundary": torch.empty(V, dtype=torch.uint8, device=dev)}
    nbytes = ctypes.c_int64()
    check(L.d3ga_loop_plan_scratch_bytes(V, F, ctypes.byref(nbytes)), "d3ga_loop_plan_scratch_bytes")
    scratch = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    with torch.no_grad():
        check(L.d3ga_loop_edge_keys(V, F, dptr(f32), dptr(keys), dptr(status), s), "d3ga_loop_edge_keys")
        sorted_keys, perm = torch.sort(keys, stable=True)
        plan = LoopPlan(f32, V, 0, 0, 0, tables, info)
        st = plan.struct(built=False)
        check(L.d3ga_loop_plan_build(ctypes.byref(st), dptr(f32), dptr(sorted_keys), dptr(perm), dptr(info), dptr(scratch), nbytes.value, s),
              "d3ga_loop_plan_build")
        E, kmax, word, _ = (int(x) for x in info.cpu().tolist())            # the one read-back
    return LoopPlan(f32, V, E, kmax, word, tables, info)


def _matrix(what, name, x, rows=None, device=None):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
        if device is not None:
            x = x.to(device)
    if not torch.is_tensor(x):
        raise ValueError(f"{what}: {name} must be a tensor or an array, got {type(x).__name__}")
    x = x.detach()
    if x.dim() == 3 and x.shape[0] == 1:
        x = x[0]
    if x.dim() != 2 or (rows is not None and x.shape[0] != rows):
        raise ValueError(f"{what}: expected {name} ({'V' if rows is None else rows},C), got {tuple(x.shape)}")
    if x.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{what}: {name} must be float32 or float64, got {x.dtype}")
    return x


def _finite(what, name, x):
    if x.numel() and not bool(torch.isfinite(x).all()):
        raise ValueError(f"{what}: {name} holds values that are not finite")


def _stencil(plan, x):
    """x (V, D) -> (V + E, D) float32"""
    D = x.shape[1]
    out = torch.empty((plan.V + plan.E, D), dtype=torch.float32, device=x.device)
    if D == 0:
        return out
    x64 = x.to(torch.float64).contiguous()
    beta = plan.beta()
    st = plan.struct()
    check(_lib.lib().d3ga_loop_subdivide(ctypes.byref(st), D, dptr(x64), dptr(beta), beta.numel(), dptr(out), dptr(plan.info[2:3]),
                                         stream_handle()), "d3ga_loop_subdivide")
    return out


def loop_subdivide(vertices, faces, attrs=None, iterations=1, plan=None):
    """Loop subdivision that carries attribute columns along -> (vertices' (V+E,3) f32, faces' (4F,3) in the dtype of `faces`,
    attrs' (V+E,C) f32 or None).  Rows 0..V-1 are the even vertices, row V + e the odd vertex of unique edge e; face f = (a, b, c)
    with odd vertices o0 on ab, o1 on bc, o2 on ca becomes rows 4f..4f+3 = (a,o0,o2), (o0,b,o1), (o2,o1,c), (o0,o1,o2).
    vertices (V,3) and attrs (V,C), float32 or float64, C >= 0; faces (F,3) int32 or int64.  `plan`: a LoopPlan of these faces
    (iterations == 1 only), else built here.  Raises ValueError for a mesh the plan flags (module docstring) and for inputs that
    are not finite."""
    what = "loop_subdivide"
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or iterations < 1:
        raise ValueError(f"{what}: iterations must be a positive integer, got {iterations!r}")
    v = _matrix(what, "vertices", vertices)
    if v.shape[1] != 3 or v.shape[0] < 1:
        raise ValueError(f"{what}: expected vertices (V,3) with V >= 1, got {tuple(v.shape)}")
    f = _as_faces(what, faces, v.device)
    a = None if attrs is None else _matrix(what, "attrs", attrs, rows=v.shape[0], device=v.device)
    if plan is not None:
        if not isinstance(plan, LoopPlan):
            raise ValueError(f"{what}: plan must be a LoopPlan, got {type(plan).__name__}")
        if iterations != 1:
            raise ValueError(f"{what}: a plan describes one level; iterations = {iterations}")
        if plan.V != v.shape[0] or plan.F != f.shape[0]:
            raise ValueError(f"{what}: the plan is of a mesh with V = {plan.V}, F = {plan.F}; this one has V = {v.shape[0]}, F = {f.shape[0]}")
    for name, t in (("faces", f), ("attrs", a)):
        if t is not None and t.device != v.device:
            raise ValueError(f"{what}: {name} are on {t.device}, vertices on {v.device}")
    require_cuda(v, f, a)
    _finite(what, "vertices", v)
    if a is not None:
        _finite(what, "attrs", a)
    dtype = f.dtype
    with torch.no_grad():
        for _ in range(int(iterations)):
            p = plan if plan is not None else loop_plan(f, v.shape[0])
            p.check()
            v = _stencil(p, v)
            if a is not None:
                a = _stencil(p, a)
            nf = torch.empty((4 * p.F, 3), dtype=torch.int32, device=v.device)
            st = p.struct()
            check(_lib.lib().d3ga_loop_faces(ctypes.byref(st), dptr(p.faces), dptr(nf), stream_handle()), "d3ga_loop_faces")
            f = nf
    return v, f.to(dtype), a


def nearest_vertex(template_vertices, template_faces, query, inflate=0.0):
    """For every query point the index of the nearest template vertex -> (n,) int64 (`Smplman.find_nn`).  inflate != 0 moves the
    template along its angle-weighted vertex normals first (`gauss_init.inflate`, trimesh's `vertex_normals` rule).  The search is
    `knn_points(K=1)`: float32 squared distances as csrc/knn_math.h defines them, ties to the lowest index."""
    what = "nearest_vertex"
    from .gauss_init import inflate as _inflate
    from .knn import knn_points
    t = _matrix(what, "template_vertices", template_vertices)
    q = _matrix(what, "query", query, device=t.device)
    if t.shape[1] != 3 or t.shape[0] < 1 or q.shape[1] != 3 or q.shape[0] < 1:
        raise ValueError(f"{what}: expected template_vertices (V,3) and query (n,3), got {tuple(t.shape)} and {tuple(q.shape)}")
    amount = float(inflate)
    if not math.isfinite(amount):
        raise ValueError(f"{what}: inflate = {amount} is not finite")
    if q.device != t.device:
        raise ValueError(f"{what}: query is on {q.device}, template_vertices on {t.device}")
    require_cuda(t, q)
    _finite(what, "template_vertices", t)
    _finite(what, "query", q)
    if amount != 0.0:
        t = _inflate(t, _as_faces(what, template_faces, t.device), amount)
    with torch.no_grad():
        return knn_points(q.float()[None], t.float()[None], K=1).idx[0, :, 0].contiguous()


class Unposed:
    """What `unpose` returns: vertices (n,3) float32 and the sticky status word (1,) int32 on the device.  Unpacks as
    (vertices, status); `check()` reads the status back and raises ValueError for a singular blend or an index outside its table."""

    def __init__(self, vertices, status):
        self.vertices, self.status = vertices, status

    def __iter__(self):
        return iter((self.vertices, self.status))

    def check(self):
        err = _status_error("unpose", int(self.status.item()))
        if err is not None:
            raise err
        return self


def unpose(vertices, joint_mats, skin, rows=None, blend_offsets=None):
    """`Smplman.unpose` in closed form: x_i = M^-1 (v_i - t / s) - blend_offsets[rows[i]], with [M t; 0 0 0 s] = sum_j w_j A_j over
    row rows[i] of the skin table, in float64, one launch; the (n,4,4) blends are never written.  -> Unposed(vertices (n,3) f32,
    status).  vertices (n,3) or (1,n,3); joint_mats (J,4,4) or (1,J,4,4); skin: the dense table (R,J), or the K-sparse pair
    (skin_idx (R,K) int32, skin_w (R,K)) of `sparse_skin_weights`; rows (n,) integers into the table (None: row i);
    blend_offsets (Vb,3) or (1,Vb,3), read at rows (None: nothing is subtracted).  Weights of 0 are skipped and the others added
    in stored order, so the dense table and its sparse form give the same bits.  |det M| or |s| below 1e-12 sets the status bit
    and the row is zeros -- never NaN or Inf."""
    what = "unpose"
    v = _matrix(what, "vertices", vertices)
    if v.shape[1] != 3 or v.shape[0] < 1:
        raise ValueError(f"{what}: expected vertices (n,3) with n >= 1, got {tuple(v.shape)}")
    n, dev = v.shape[0], v.device
    A = joint_mats
    if not torch.is_tensor(A) or A.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{what}: joint_mats must be a float32 or float64 tensor")
    A = A.detach()
    if A.dim() == 4 and A.shape[0] == 1:
        A = A[0]
    if A.dim() != 3 or tuple(A.shape[1:]) != (4, 4) or A.shape[0] < 1:
        raise ValueError(f"{what}: expected joint_mats (J,4,4), got {tuple(joint_mats.shape)}")
    J = A.shape[0]
    idx = None
    if isinstance(skin, (tuple, list)):
        if len(skin) != 2 or not all(torch.is_tensor(t) for t in skin):
            raise ValueError(f"{what}: a sparse skin is the pair (skin_idx, skin_w) of tensors")
        idx, w = skin[0].detach(), skin[1].detach()
        if idx.dim() != 2 or idx.shape != w.shape or idx.shape[0] < 1 or idx.shape[1] < 1:
            raise ValueError(f"{what}: expected skin_idx and skin_w of one shape (R,K), got {tuple(idx.shape)} and {tuple(w.shape)}")
        if idx.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{what}: skin_idx must be int32 or int64, got {idx.dtype}")
    else:
        w = _matrix(what, "skin", skin)
        if w.shape[1] != J or w.shape[0] < 1:
            raise ValueError(f"{what}: expected the dense skin table (R,{J}), got {tuple(w.shape)}")
    if w.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{what}: skin weights must be float32 or float64, got {w.dtype}")
    R, K = w.shape
    if R * K > 2 ** 31 - 1:
        raise ValueError(f"{what}: the skin table has {R * K} entries, more than 2^31 - 1")
    if rows is None:
        if R != n:
            raise ValueError(f"{what}: without rows the skin table needs {n} rows, it has {R}")
    else:
        if not torch.is_tensor(rows) or rows.dim() != 1 or rows.shape[0] != n or rows.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{what}: rows must be an int32 or int64 tensor ({n},)")
    bs = None
    if blend_offsets is not None:
        bs = _matrix(what, "blend_offsets", blend_offsets, device=dev)
        if bs.shape[1] != 3 or bs.shape[0] < 1:
            raise ValueError(f"{what}: expected blend_offsets (Vb,3), got {tuple(bs.shape)}")
    for name, t in (("joint_mats", A), ("skin", w), ("skin_idx", idx), ("rows", rows), ("blend_offsets", bs)):
        if t is not None and t.device != dev:
            raise ValueError(f"{what}: {name} is on {t.device}, vertices on {dev}")
    require_cuda(v, A, w, idx, rows, bs)
    _finite(what, "vertices", v)
    _finite(what, "joint_mats", A)
    _finite(what, "skin", w)
    if bs is not None:
        _finite(what, "blend_offsets", bs)
    v64, A64 = v.to(torch.float64).contiguous(), A.to(torch.float64).contiguous()
    w = w.contiguous()
    idx = None if idx is None else idx.clamp(-1, 2 ** 31 - 1).to(torch.int32).contiguous()
    rows64 = None if rows is None else rows.detach().to(torch.int64).contiguous()
    bs64 = None if bs is None else bs.to(torch.float64).contiguous()
    out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.no_grad():
        check(_lib.lib().d3ga_unpose(n, J, R, K, dptr(v64), dptr(A64), dptr(w), 1 if w.dtype == torch.float64 else 0, dptr(idx), dptr(rows64),
                                     dptr(bs64), 0 if bs64 is None else bs64.shape[0], dptr(out), dptr(status), stream_handle()), "d3ga_unpose")
    return Unposed(out, status)


def star_pose(layer):
    """The layer's output at the reference's star pose (`Smplman.get_star_pose(return_Tbs=True)`): poses[:,5] = pi/6,
    poses[:,8] = -pi/6, zero shapes, expression, Rh and Th -> (vertices (1,V,3), T (1,V,4,4), A (1,J,4,4), bs (1,V,3))."""
    dev = layer.v_template.device
    poses = torch.zeros((1, layer.NUM_POSES), dtype=torch.float32, device=dev)
    if layer.NUM_POSES < 9:
        raise ValueError(f"star_pose: the layer takes {layer.NUM_POSES} pose values, the star pose sets entries 5 and 8")
    poses[:, 5] = np.pi / 6
    poses[:, 8] = -np.pi / 6
    zeros3 = torch.zeros((1, 3), dtype=torch.float32, device=dev)
    shapes = torch.zeros((1, max(int(getattr(layer, "n_shape", 10)), 1)), dtype=torch.float32, device=dev)
    n_expr = int(getattr(layer, "n_expr", 10))
    expression = torch.zeros((1, n_expr), dtype=torch.float32, device=dev) if n_expr > 0 else None
    with torch.no_grad():
        return layer(poses=poses, shapes=shapes, Rh=zeros3, Th=zeros3.clone(), expression=expression)


def bind_body_template(layer, inflate=0.0, densify=True, offset=None):
    """What `Smplman.create_body_model` leaves on `self` -> TemplateBinding(body_template_vertices (1,V',3) f32, body_template_faces
    (F',3), skin_weights (V',J) f32, nn_ids (V',) int64): the star-pose vertices (+ offset (V,3), `data.smplx_offset`) are
    subdivided together with `layer.weights` (densify=False: taken as they are); every dense vertex finds the nearest ORIGINAL
    vertex of the star-pose template inflated by `inflate`; the dense vertices are unposed with the dense table at rows nn_ids."""
    what = "bind_body_template"
    verts, _, A, bs = star_pose(layer)
    v, faces, weights = verts[0], layer.faces_tensor, layer.weights
    template = v
    if offset is not None:
        off = _matrix(what, "offset", offset, rows=v.shape[0], device=v.device)
        if off.shape[1] != 3:
            raise ValueError(f"{what}: expected offset ({v.shape[0]},3), got {tuple(off.shape)}")
        _finite(what, "offset", off)
        template = v = (v.double() + off.to(v.device).double()).float()      # `v += delta` on the float32 array: one rounding
    if densify:
        nv, nf, nw = loop_subdivide(v, faces, weights, iterations=1)
    else:
        nv, nf, nw = v.float().contiguous(), faces, weights.float().contiguous()
    nn_ids = nearest_vertex(template, faces, nv, inflate)
    vtn = unpose(nv, A[0], nw, nn_ids, bs[0]).check().vertices
    return TemplateBinding(vtn[None], nf, nw, nn_ids)


def bind_cage(layer, binding, cage_vertices, inflate):
    """What `CageSmpl.create_cage_model` leaves on `self` for one cage -> CageBinding(body_template_vertices (1,Vc,3) f32, nn_ids
    (Vc,) int64, skin_idx (Vc,K) int32, skin_w (Vc,K) f32).  nn_ids index the ORIGINAL star-pose template (inflated by `inflate`)
    while `binding.skin_weights` is the SUBDIVIDED table, as in the reference: its first V rows are the even rows, so the cage is
    skinned by the smoothed weights of the even vertices.  (skin_idx, skin_w) are those rows in the K-sparse layout `lbs_cage`
    takes, i.e. `sparse_skin_weights(binding.skin_weights, rows=nn_ids)`."""
    what = "bind_cage"
    from .cage_deform import sparse_skin_weights
    if not isinstance(binding, TemplateBinding):
        raise ValueError(f"{what}: binding must be the TemplateBinding of bind_body_template, got {type(binding).__name__}")
    cage = _matrix(what, "cage_vertices", cage_vertices, device=layer.v_template.device)
    if cage.shape[1] != 3 or cage.shape[0] < 1:
        raise ValueError(f"{what}: expected cage_vertices (Vc,3), got {tuple(cage.shape)}")
    verts, _, A, bs = star_pose(layer)
    nn_ids = nearest_vertex(verts[0], layer.faces_tensor, cage, inflate)
    vtn = unpose(cage.float(), A[0], binding.skin_weights, nn_ids, bs[0]).check().vertices
    skin_idx, skin_w = sparse_skin_weights(binding.skin_weights, rows=nn_ids)
    return CageBinding(vtn[None], nn_ids, skin_idx, skin_w)


def bind_cage_skin(template_vertices, template_faces, cage_vertices, inflate, skin_weights, skin_indices):
    """Goliath's `create_cage_skin_weights` -> (cage_weights (Vc,K), cage_indices (Vc,K), cage_to_body_vertex (Vc,) int64): the rows
    of the template's K-sparse skin at the nearest vertex of the template inflated by `inflate`."""
    what = "bind_cage_skin"
    for name, t in (("skin_weights", skin_weights), ("skin_indices", skin_indices)):
        if not torch.is_tensor(t) or t.dim() != 2:
            raise ValueError(f"{what}: {name} must be a tensor (V,K)")
    V = _matrix(what, "template_vertices", template_vertices).shape[0]
    if skin_weights.shape != skin_indices.shape or skin_weights.shape[0] != V:
        raise ValueError(f"{what}: skin_weights {tuple(skin_weights.shape)} and skin_indices {tuple(skin_indices.shape)} must both have a "
                         f"row per template vertex ({V})")
    require_cuda(skin_weights, skin_indices)
    ids = nearest_vertex(template_vertices, template_faces, cage_vertices, inflate)
    return skin_weights[ids, :], skin_indices[ids, :], ids
