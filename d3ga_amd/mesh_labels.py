"""Part-label transfer onto the body mesh (csrc/mesh_labels.hip): what makes `face_to_label.npy`, the asset
`CageSmpl.__init__` / `CageBlue.__init__` load first, and the ring growth every cage runs on it -- in integer HIP kernels whose
results do not depend on scheduling.

    lib/segmentation.py:59-74   Renderer.forward (the scatter `colors[ids] += rgb`)     LabelTransfer.add / .add_fragments
    lib/segmentation.py:112-123 Segmenter.majority_vote                                 LabelTransfer.labels / majority_vote
    utils/mesh_utils.py:345-360 median_filter_mesh                                      LabelTransfer.labels / median_filter_mesh
    lib/cage.py:131-153         CageBase.grow_mask_region                               grow_mask_region

The rules are pinned by csrc/mesh_labels_math.h, whose g++ build gives the kernels' bytes, and against the reference's own
functions run on the CPU (tests/golden/mesh_labels_cases.npz).  Face neighbours follow trimesh's `face_adjacency` rule -- two
different faces that share an undirected edge occurring in exactly two faces -- built here with numpy, once: parity with trimesh
unpinned (the goldens carry the adjacency their generator built by this rule).

Two departures from the reference, both deliberate.  Every view of a batch votes on its own: the reference shares `colors` over
the batch, so at B > 1 the labels of different views are added into each other; at B = 1, its default, the results are the same.
A face without neighbours keeps its own label under the median, where the reference raises KeyError.

Forward only, no gradient.  GPU tensors only; no launch synchronises with the host."""
import numpy as np
import torch

from . import _lib
from ._lib import D3GAError, check, dptr, require_cuda, stream_handle
from .mesh_render import MeshCameras, MeshScratch, MeshTopology, rasterize_meshes


class FaceNeighbours(torch.Tensor):
    """The (F,3) int32 neighbour table as its own tensor type, so that it is never mistaken for a faces array (same shape, same
    dtype).  What `face_neighbours` returns; `.clone()`, `.to()`, `.cpu()` and save / load keep the type."""


def _faces_array(what, faces):
    f = faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)
    if f.ndim == 3 and f.shape[0] == 1:
        f = f[0]
    if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1:
        raise ValueError(f"{what}: expected faces (F,3) or (1,F,3) with F >= 1, got {tuple(f.shape)}")
    if f.dtype.kind not in "iu":
        raise ValueError(f"{what}: faces must be integers, got {f.dtype}")
    f = f.astype(np.int64)
    if f.min() < 0 or f.max() >= 2 ** 31 - 1 or len(f) > (2 ** 31 - 1) // 3:
        raise ValueError(f"{what}: face indices must lie in [0, 2^31 - 1) and 3 F must stay below 2^31")
    return f


def _table_from_pairs(what, pairs, F):
    """rows (a, b) of face pairs -> (F,3) int32, -1 padded: b among a's entries and a among b's, once per row"""
    pairs = np.asarray(pairs).reshape(-1, 2).astype(np.int64)
    if pairs.size and (pairs.min() < 0 or pairs.max() >= F):
        raise ValueError(f"{what}: the adjacency names face {int(pairs.max() if pairs.max() >= F else pairs.min())}, there are {F}")
    a, b = np.concatenate([pairs[:, 0], pairs[:, 1]]), np.concatenate([pairs[:, 1], pairs[:, 0]])
    order = np.argsort(a, kind="stable")
    a, b = a[order], b[order]
    counts = np.bincount(a, minlength=F)
    if counts.size and counts.max() > 3:
        raise ValueError(f"{what}: face {int(counts.argmax())} has {int(counts.max())} neighbours; a triangle has three edges")
    table = np.full((F, 3), -1, np.int32)
    table[a, np.arange(len(a)) - (np.cumsum(counts) - counts)[a]] = b
    return table


def _table_from_faces(what, f):
    F = len(f)
    ends = np.stack([f, np.roll(f, -1, axis=1)], axis=-1).reshape(-1, 2)              # edge 3 f + e = (v_e, v_(e+1) % 3)
    key = ends.min(1) * (int(f.max()) + 1) + ends.max(1)
    order = np.argsort(key, kind="stable")
    _, start, count = np.unique(key[order], return_index=True, return_counts=True)
    start = start[count == 2]
    pairs = np.stack([order[start] // 3, order[start + 1] // 3], axis=1)
    return _table_from_pairs(what, pairs[pairs[:, 0] != pairs[:, 1]], F)


def _same_device(a, b):
    a, b = torch.device(a), torch.device(b)
    return a.type == b.type and (a.index == b.index or a.index is None or b.index is None)


def _upload(t, device):
    """a host array's tensor -> `device`; the kernels have no CPU fallback, so without a GPU this is the package's usual error"""
    if torch.device(device).type == "cuda" and not torch.cuda.is_available():
        raise D3GAError("d3ga_amd ops run on the GPU only and no GPU is available; there is no CPU fallback")
    return t.to(device)


def _tagged(table):
    return table.as_subclass(FaceNeighbours)


def face_neighbours(faces, device="cuda"):
    """faces (F,3) or (1,F,3), tensor or array -> the (F,3) int32 neighbour table on `device`, padded with -1: per face the faces
    across those of its three edges that occur in exactly two faces (an edge in one face, or in three or more, gives nothing; a
    pair that shares two such edges appears twice, as in trimesh).  Init-time work on the host, as mesh_render's vertex -> face
    lists.  Returns a `FaceNeighbours`, the tensor type median_filter_mesh / grow_mask_region take as a table."""
    what = "face_neighbours"
    return _tagged(_upload(torch.from_numpy(_table_from_faces(what, _faces_array(what, faces))), device))


def _neighbours(what, mesh_or_neighbours, device):
    """A FaceNeighbours table, a faces array or tensor (any other (F,3) array IS a faces array), or an object with `.faces` (and
    `.face_adjacency`, used if present) -> the table on `device`."""
    x = mesh_or_neighbours
    if isinstance(x, FaceNeighbours):
        if x.dim() != 2 or x.shape[1] != 3 or x.shape[0] < 1 or x.dtype != torch.int32 or not x.is_contiguous():
            raise ValueError(f"{what}: a neighbour table is a contiguous int32 tensor (F,3), got {tuple(x.shape)} {x.dtype}")
        if not _same_device(x.device, device):
            raise ValueError(f"{what}: the neighbour table is on {x.device}, the data on {device}")
        return x
    if hasattr(x, "faces"):
        f = _faces_array(what, x.faces)
        pairs = getattr(x, "face_adjacency", None)
        table = _table_from_faces(what, f) if pairs is None else _table_from_pairs(what, pairs.detach().cpu().numpy() if torch.is_tensor(pairs) else pairs, len(f))
        return _tagged(_upload(torch.from_numpy(table), device))
    if not torch.is_tensor(x) and not isinstance(x, np.ndarray):
        raise ValueError(f"{what}: expected a neighbour table, a faces array or an object with .faces, got {type(x).__name__}")
    return _tagged(_upload(torch.from_numpy(_table_from_faces(what, _faces_array(what, x))), device))


def _per_face(what, name, x, F, device):
    """a (F,) array or tensor -> (tensor on `device`, was it numpy)"""
    was_numpy = not torch.is_tensor(x)
    t = torch.from_numpy(np.ascontiguousarray(x)) if was_numpy else x.detach()
    if t.dim() != 1 or t.shape[0] != F:
        raise ValueError(f"{what}: expected {name} ({F},), got {tuple(t.shape)}")
    return (_upload(t, device) if was_numpy else t), was_numpy


def _table_for(what, mesh_or_neighbours, data):
    """the table, on the device of the data (a tensor), else of a ready table, else the current GPU"""
    if torch.is_tensor(data):
        dev = data.device
    elif isinstance(mesh_or_neighbours, FaceNeighbours):
        dev = mesh_or_neighbours.device
    else:
        dev = torch.device("cuda")
    return _neighbours(what, mesh_or_neighbours, dev), dev


def _majority(hist, out):
    F, L = hist.shape
    check(_lib.lib().d3ga_label_majority(F, L, dptr(hist), dptr(out), stream_handle()), "d3ga_label_majority")


def _median(table, labels, out):
    check(_lib.lib().d3ga_label_median(labels.shape[0], dptr(table), dptr(labels), dptr(out), stream_handle()), "d3ga_label_median")


def majority_vote(part_per_face=None, *, hist=None, n_labels=None):
    """Segmenter.majority_vote: part_per_face (F, n) integer labels, one column per view, 0 (or less) = no vote -> (F,) the most
    frequent label above 0 of every row, ties to the smallest, 0 without a vote.  On host or device; returns numpy for numpy.
    The rows are histogrammed on the device with torch (plumbing), the pick is the kernel's.  Alternatively hist=(F,L) int32
    counts, as LabelTransfer.counts() returns them.  n_labels: columns of the histogram, default max + 1; at most 32."""
    what = "majority_vote"
    if (part_per_face is None) == (hist is None):
        raise ValueError(f"{what}: give part_per_face or hist=")
    x = part_per_face if hist is None else hist
    was_numpy = not torch.is_tensor(x)
    t = torch.from_numpy(np.ascontiguousarray(x)) if was_numpy else x.detach()
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{what}: expected a non-empty 2-D array, got {tuple(t.shape)}")
    if t.is_floating_point() or t.dtype == torch.bool or t.is_complex():
        raise ValueError(f"{what}: labels and counts are integers, got {t.dtype}")
    if hist is not None:
        if t.shape[1] > _lib.LABELS_MAX:
            raise ValueError(f"{what}: a histogram has at most {_lib.LABELS_MAX} columns, got {t.shape[1]}")
        if was_numpy:
            t = _upload(t, "cuda")
        require_cuda(t)
        counts = t.to(torch.int32).contiguous()
    else:
        top = int(t.max())
        L = max(top + 1, 2) if n_labels is None else int(n_labels)
        if not 1 <= L <= _lib.LABELS_MAX or top >= L:
            raise ValueError(f"{what}: labels up to {top} with n_labels = {L}; at most {_lib.LABELS_MAX} columns, every label below n_labels")
        if was_numpy:
            t = _upload(t, "cuda")
        require_cuda(t)
        idx = t.clamp(min=0).long()
        counts = torch.zeros(t.shape[0], L, dtype=torch.int32, device=t.device).scatter_add_(1, idx, torch.ones_like(idx, dtype=torch.int32))
    out = torch.empty(counts.shape[0], dtype=torch.int32, device=counts.device)
    with torch.no_grad():
        _majority(counts, out)
    return out.cpu().numpy().astype(np.int64) if was_numpy else out


def median_filter_mesh(mesh_or_neighbours, labels):
    """utils/mesh_utils.py::median_filter_mesh: every face gets the median of its neighbours' labels (two neighbours: (a + b) // 2,
    labels are not negative); a face without neighbours keeps its own.  mesh_or_neighbours: a table from face_neighbours, a faces
    array, or any object with `.faces` (`.face_adjacency` is used if present).  labels (F,) integers; numpy in, numpy out."""
    what = "median_filter_mesh"
    table, dev = _table_for(what, mesh_or_neighbours, labels)
    t, was_numpy = _per_face(what, "labels", labels, table.shape[0], dev)
    if t.is_floating_point() or t.dtype == torch.bool:
        raise ValueError(f"{what}: labels are integers, got {t.dtype}")
    require_cuda(table, t)
    src = t.to(torch.int32).contiguous()
    out = torch.empty_like(src)
    with torch.no_grad():
        _median(table, src, out)
    return out.cpu().numpy().astype(np.int64) if was_numpy else out.to(t.dtype)


def grow_mask_region(mesh_or_neighbours, mask, n_rings=1):
    """CageBase.grow_mask_region: n_rings times, every face i with 0 < #{n in N(i): mask[n]} < len(N(i)) marks all its neighbours.
    The reference carries `mask` and `region`; they start equal and receive the same faces in every ring, so one is carried.
    mask (F,) bool (or uint8); numpy in, numpy out.  All rings are enqueued by one call."""
    what = "grow_mask_region"
    n_rings = int(n_rings)
    if not 0 <= n_rings <= _lib.LABEL_RINGS_MAX:
        raise ValueError(f"{what}: n_rings = {n_rings} outside 0 .. {_lib.LABEL_RINGS_MAX}")
    table, dev = _table_for(what, mesh_or_neighbours, mask)
    t, was_numpy = _per_face(what, "mask", mask, table.shape[0], dev)
    if t.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"{what}: mask must be bool or uint8, got {t.dtype}")
    require_cuda(table, t)
    F = t.shape[0]
    src = t.to(torch.uint8).contiguous()
    out = torch.empty_like(src)
    scratch = torch.empty(2 * F, dtype=torch.uint8, device=src.device) if n_rings >= 2 else None
    with torch.no_grad():
        check(_lib.lib().d3ga_label_grow(F, n_rings, dptr(table), dptr(src), dptr(out), dptr(scratch), stream_handle()), "d3ga_label_grow")
    return out.cpu().numpy().astype(bool) if was_numpy else out.to(t.dtype)


class LabelTransfer:
    """The accumulation of Segmenter.run: views vote for the part label of every face they show, then `labels()`.

        lt = LabelTransfer(faces, n_labels=5, B=1, H=H, W=W)
        for batch in loader:                                   # up to 512 in the reference
            lt.add(cameras, vertices, batch["seg_part"])       # rasterize_meshes + the two vote launches
        lt.check(); face_to_label = lt.labels()                # majority, then the median filter

    Per view and face the vote is the label at the LAST pixel in raster order among those the face wins (what the reference's
    index-put keeps on the CPU; on a GPU the reference's result depends on scheduling, this one does not).  Owns `hist` (F,
    n_labels) int32, the (B,F) vote scratch (cleared once, here; every call leaves it clean), the status word and a MeshScratch.
    Nothing is allocated after construction and `add_fragments` never synchronises: it is capturable in torch.cuda.graph.
    n_verts: vertices of the meshes `add` will be given (default: what the faces name)."""

    def __init__(self, faces, n_labels, B, H, W, device="cuda", n_verts=None):
        what = "LabelTransfer"
        self.topology = faces if isinstance(faces, MeshTopology) else MeshTopology(torch.as_tensor(_faces_array(what, faces)))
        n_labels, B, H, W = int(n_labels), int(B), int(H), int(W)
        F = self.topology.F
        if F < 1:
            raise ValueError(f"{what}: no faces")
        if not 1 <= n_labels <= _lib.LABELS_MAX:
            raise ValueError(f"{what}: n_labels = {n_labels} outside 1 .. {_lib.LABELS_MAX}")
        if not (1 <= B <= 65535 and 1 <= H <= _lib.MESH_MAX_SIDE and 1 <= W <= _lib.MESH_MAX_SIDE) or B * F >= 2 ** 31 or F * n_labels >= 2 ** 31:
            raise ValueError(f"{what}: B, H, W = {(B, H, W)} with {F} faces: 1 <= B <= 65535, sides 1 .. {_lib.MESH_MAX_SIDE}, B F and F n_labels < 2^31")
        V = self.topology.min_verts if n_verts is None else int(n_verts)
        if V < self.topology.min_verts:
            raise ValueError(f"{what}: the faces name vertex {self.topology.min_verts - 1}, n_verts = {V}")
        self.F, self.L, self.B, self.H, self.W = F, n_labels, B, H, W
        self._flags = 0                                       # D3GA_LABEL_EVERY_PIXEL for tools/time_mesh_labels.py; same results
        self.hist = torch.zeros(F, n_labels, dtype=torch.int32, device=device)
        self.device = self.hist.device
        self.neighbours = _tagged(torch.from_numpy(_table_from_faces(what, self.topology._host.astype(np.int64))).to(self.device))
        self.cells = torch.zeros(B, F, dtype=torch.int32, device=self.device)
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._voted = torch.zeros(F, dtype=torch.int32, device=self.device)
        self.scratch = MeshScratch(B, V, F, H, W, device=self.device)

    def add_fragments(self, pix_to_face, seg_part):
        """pix_to_face (B,H,W) int32, contiguous, per-mesh face indices as rasterize_meshes writes them (-1: nothing; values
        >= F are ignored); seg_part (B,1,H,W) or (B,H,W), int32 or uint8, as prepare_actorshq hands it out -- rows may be padded
        and frames strided, elements of a row are dense.  Two launches."""
        what = "LabelTransfer.add_fragments"
        B, H, W = self.B, self.H, self.W
        if not torch.is_tensor(pix_to_face) or tuple(pix_to_face.shape) != (B, H, W) or pix_to_face.dtype != torch.int32 or \
                not pix_to_face.is_contiguous():
            raise ValueError(f"{what}: pix_to_face must be a contiguous int32 tensor {(B, H, W)}, got "
                             f"{(tuple(pix_to_face.shape), pix_to_face.dtype) if torch.is_tensor(pix_to_face) else type(pix_to_face).__name__}")
        if not torch.is_tensor(seg_part):
            raise ValueError(f"{what}: seg_part must be a tensor, got {type(seg_part).__name__}")
        part = seg_part[:, 0] if seg_part.dim() == 4 and seg_part.shape[1] == 1 else seg_part
        if tuple(part.shape) != (B, H, W):
            raise ValueError(f"{what}: expected seg_part {(B, 1, H, W)} or {(B, H, W)}, got {tuple(seg_part.shape)}")
        if part.dtype not in (torch.int32, torch.uint8):
            raise ValueError(f"{what}: seg_part must be int32 or uint8, got {part.dtype}")
        elem = part.element_size()
        sb, sh, sw = part.stride()
        if W > 1 and sw != 1:
            raise ValueError(f"{what}: seg_part has strides {tuple(seg_part.stride())}: the elements of a row must be dense")
        pitch = sh * elem if H > 1 else W * elem
        frame = sb * elem if B > 1 else 0
        if pitch < W * elem or (B > 1 and frame < (H - 1) * pitch + W * elem):
            raise ValueError(f"{what}: seg_part has strides {tuple(seg_part.stride())}: rows or frames overlap")
        for name, t in (("pix_to_face", pix_to_face), ("seg_part", part)):
            if t.device != self.device:
                raise ValueError(f"{what}: {name} is on {t.device}, the owner on {self.device}")
        require_cuda(pix_to_face, part)
        with torch.no_grad():
            check(_lib.lib().d3ga_label_vote(B, self.F, self.L, H, W, dptr(pix_to_face), dptr(part), int(part.dtype == torch.uint8), pitch, frame,
                                             dptr(self.cells), dptr(self.hist), dptr(self.status), self._flags, stream_handle()),
                  "d3ga_label_vote")

    def add(self, cameras, vertices, seg_part):
        """One batch of Segmenter.run: `rasterize_meshes` into the owned MeshScratch, then `add_fragments`.  cameras: the
        MeshCameras of mesh_render.to_cameras, or what compat/pytorch3d's cameras_from_opencv_projection returns
        (lib/segmentation.py:41-47); vertices (B,V,3) float32."""
        what = "LabelTransfer.add"
        if not isinstance(cameras, MeshCameras):
            if not hasattr(cameras, "mesh_cameras"):
                raise ValueError(f"{what}: cameras must be MeshCameras or come from cameras_from_opencv_projection, got {type(cameras).__name__}")
            cameras = cameras.mesh_cameras((self.H, self.W), self.device)
        if (cameras.H, cameras.W) != (self.H, self.W):
            raise ValueError(f"{what}: the cameras render {(cameras.H, cameras.W)}, the owner was built for {(self.H, self.W)}")
        fragments = rasterize_meshes(cameras, vertices, self.topology, scratch=self.scratch)
        self.add_fragments(fragments.pix_to_face, seg_part)

    def counts(self):
        """The (F, n_labels) int32 histogram (the owner's tensor, not a copy): column 0 counts the views that saw the face as
        background."""
        return self.hist

    def labels(self, median=True, out=None):
        """(F,) int32: per face the label above 0 with the most votes (ties to the smallest, 0 without a vote), then, with
        `median`, the median over the face's neighbours.  out: a contiguous int32 (F,) tensor to write into."""
        what = "LabelTransfer.labels"
        if out is None:
            out = torch.empty(self.F, dtype=torch.int32, device=self.device)
        elif not torch.is_tensor(out) or tuple(out.shape) != (self.F,) or out.dtype != torch.int32 or not out.is_contiguous() or \
                out.device != self.device:
            raise ValueError(f"{what}: out must be a contiguous int32 tensor {(self.F,)} on {self.device}")
        require_cuda(self.hist, out)
        with torch.no_grad():
            _majority(self.hist, self._voted if median else out)
            if median:
                _median(self.neighbours, self._voted, out)
        return out

    def check(self):
        """One read-back: raises ValueError if any vote so far named a label outside [0, n_labels) (such votes count nothing)."""
        if int(self.status.item()) & _lib.LABEL_STATUS_RANGE:
            raise ValueError(f"LabelTransfer: a label image held a value outside [0, {self.L}) at a pixel that voted")

    def reset(self):
        """A new accumulation: clears the histogram and the status word."""
        self.hist.zero_()
        self.status.zero_()
