"""Per-frame state addressed by a DEVICE index: the latent frame codes and the refined SMPL-X parameters of the reference's
GarmentNet, in a form that a captured step (graph.CapturedStep) follows from replay to replay (csrc/frame_state.hip).

Drop-ins for
    models/embeddings.py:13-36            Embedding           (models/garment_net.py:18, 39-41, 163-178)
    the three nn.ParameterDict of         RowCache, FramePoses (models/garment_net.py:87-107, 116-119, 211-235)
    prepare_opt_tensors / update_batch
GPU tensors only.  The frame is an int32 device cell; put it in `CapturedStep(slots={"frame": cell})`:

    frame = torch.zeros(1, dtype=torch.int32, device="cuda")
    poses.attach(opt)
    def step():
        poses.select(frame)
        code = emb(frame)[0, :, 0, 0]
        ...
        loss.backward()
        opt.step()
    cap = CapturedStep(step, params=params, slots={"frame": frame}, camera=slot)
    cap.replay(camera=batch, frame=torch.tensor([poses.index(key)], dtype=torch.int32))

Call `poses.flush()` and `poses.check()` before a checkpoint.
"""
import ctypes
from collections import OrderedDict

import torch
from torch import nn

from . import _lib
from ._lib import D3GAError, check, dptr, require_cuda, stream_handle
from .calibration import _cam_cells_for

__all__ = ["code_lookup", "Embedding", "RowCache", "FramePoses", "convert_optimizer_state"]


def _host_indices(idx):
    """idx given on the host as a list of ints (None: idx lives on the device)"""
    if torch.is_tensor(idx):
        if idx.is_cuda:
            return None
        if idx.is_floating_point() or idx.dtype == torch.bool:
            raise TypeError(f"an index must be an integer, got {idx.dtype}")
        return [int(i) for i in idx.reshape(-1).tolist()]
    if isinstance(idx, (list, tuple)):
        return [int(i) for i in idx]
    return [int(idx)]


# ---- the latent codes ------------------------------------------------------------------------------------------------------
class _CodeLookup(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weight, cells, max_norm):
        n, d = weight.shape
        b = cells.numel()
        out = torch.empty(b, d, dtype=torch.float32, device=weight.device)
        check(_lib.lib().d3ga_code_lookup_fwd(dptr(weight), dptr(cells), n, d, b, max_norm, dptr(out), stream_handle()),
              "d3ga_code_lookup_fwd")
        if max_norm > 0:
            # the kernel may have scaled rows of `weight` in place: caches keyed by the version counter must see it
            torch.autograd.graph.increment_version(weight)
        ctx.save_for_backward(cells)
        ctx.shape = (n, d, b)
        return out

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        (cells,) = ctx.saved_tensors
        n, d, b = ctx.shape
        g = g.float().contiguous()
        dtable = torch.empty(n, d, dtype=torch.float32, device=g.device)       # written whole by the one launch
        check(_lib.lib().d3ga_code_lookup_bwd(dptr(g), dptr(cells), n, d, b, dptr(dtable), stream_handle()), "d3ga_code_lookup_bwd")
        return dtable, None, None


def code_lookup(weight, idx, max_norm=None):
    """F.embedding(idx, weight, max_norm=max_norm) for up to 16 indices -> (B, D), in one launch per direction.

    weight (N,D) float32, contiguous.  idx: an int, a sequence or CPU tensor of ints, an integer device tensor, or a (B,) int32
    device cell -- only the last is read when the kernel RUNS, so a captured step follows the cell; everything else is turned
    into a constant cell when the call is issued.  Every index is clamped into [0, N-1] (the reference clamps the top).
    With max_norm, torch's embedding_renorm_ runs first, under no_grad and IN PLACE on `weight`: every distinct looked-up row
    with an L2 norm > max_norm is multiplied by max_norm / (norm + 1e-7); the version counter of `weight` is bumped.
    Differentiable in weight: the dense (N,D) gradient nn.Embedding produces, every element written, bit-reproducible."""
    if weight.dim() != 2:
        raise ValueError(f"code_lookup: expected weight (N,D), got {tuple(weight.shape)}")
    n, d = weight.shape
    host = _host_indices(idx)
    b = idx.numel() if host is None else len(host)
    if not 1 <= b <= _lib.CODE_MAX_B:
        raise ValueError(f"code_lookup: {b} indices, at most {_lib.CODE_MAX_B} (and at least one) per call")
    if not 1 <= d <= _lib.CODE_MAX_D or n < 1:
        raise ValueError(f"code_lookup: weight {tuple(weight.shape)}, expected N >= 1 and 1 <= D <= {_lib.CODE_MAX_D}")
    require_cuda(weight)
    if weight.dtype != torch.float32 or not weight.is_contiguous():
        raise ValueError("code_lookup: weight must be float32 and contiguous (the renorm writes it in place)")
    if host is None:
        if idx.is_floating_point() or idx.dtype == torch.bool:
            raise TypeError(f"code_lookup: an index must be an integer, got {idx.dtype}")
        require_cuda(idx)
        cells = idx.reshape(-1).to(torch.int32).contiguous()
    else:
        cells = _cam_cells_for(tuple(min(max(i, 0), n - 1) for i in host), b, n, weight.device, "code_lookup")
    return _CodeLookup.apply(weight, cells, float(max_norm) if max_norm is not None and max_norm > 0 else 0.0)


class _Codes(nn.Module):
    """Holds the table as `weight`, where nn.Embedding keeps it (`embeddings.frame_embs.weight` of a reference checkpoint)."""

    def __init__(self, n, d, std):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(n, d).normal_(0.0, std))


class Embedding(nn.Module):
    """models/embeddings.py:13-36: same constructor, attributes, parameter (`frame_embs.weight`, normal(0, std), max_norm =
    float(n_dims)) and results; reference checkpoints load with strict=True.  Created on the CPU; follows .cuda() / .to()."""

    def __init__(self, n_frames, n_dims, height=1, width=1, std=0.1, **kwargs):
        super().__init__()
        self.n_frames, self.n_dims, self.height, self.width = n_frames, n_dims, height, width
        self.max_norm = float(n_dims)
        self.frame_embs = _Codes(n_frames, height * width * n_dims, std)
        self._avg = (None, None)

    def forward(self, idxs):
        """idxs: (B,) indices as `code_lookup` takes them -> (B, n_dims, height, width)"""
        out = code_lookup(self.frame_embs.weight, idxs, self.max_norm)
        return out.reshape(out.shape[0], self.n_dims, self.height, self.width)

    def average(self):
        """weight.mean(0, keepdims=True) -> (1, height width n_dims), detached (the reference takes it at evaluation only).
        Computed once per (weight storage, version, replay epoch): an evaluation loop pays for it once."""
        w = self.frame_embs.weight
        require_cuda(w)
        key = (w.data_ptr(), w._version, _lib.replay_epoch[0])
        if self._avg[0] != key:
            n, d = w.shape
            need = ctypes.c_int64()
            check(_lib.lib().d3ga_table_mean_scratch_bytes(n, d, ctypes.byref(need)), "d3ga_table_mean_scratch_bytes")
            scratch = torch.empty(need.value // 8, dtype=torch.float64, device=w.device)
            out = torch.empty(1, d, dtype=torch.float32, device=w.device)
            src = w.detach().contiguous()
            check(_lib.lib().d3ga_table_mean(dptr(src), n, d, dptr(out), dptr(scratch), stream_handle()), "d3ga_table_mean")
            self._avg = (key, out)
        return self._avg[1]

    def median(self):
        return self.frame_embs.weight.median(0, keepdims=True)


# ---- one staged row per table ----------------------------------------------------------------------------------------------
def _select_cell(idx, n_rows, device, what):
    """The (1,) int32 device cell of a select: host indices are checked here, a device cell is checked by the kernel."""
    if torch.is_tensor(idx) and idx.is_cuda:
        if idx.numel() != 1:
            raise ValueError(f"{what}: one row is staged per cache, got {idx.numel()} indices")
        if idx.dtype != torch.int32:
            raise ValueError(f"{what}: a device index must be an int32 cell, got {idx.dtype}")
        require_cuda(idx)
        return idx.reshape(1)
    host = _host_indices(idx)
    if len(host) != 1:
        raise ValueError(f"{what}: one row is staged per cache, got {len(host)} indices")
    if not 0 <= host[0] < n_rows:
        raise IndexError(f"{what}: row {host[0]} outside [0, {n_rows})")
    if device.type != "cuda":
        raise D3GAError(f"{what} runs on the GPU only (rows on {device}); there is no CPU fallback")
    return _cam_cells_for(host[0], 1, n_rows, device, what)


class _Cells:
    """Launches of one select group: the pairs of one RowCache, or of the three caches of a FramePoses."""

    def __init__(self, caches, what):
        self.caches, self.what = caches, what
        self._desc = (None, None)

    def cells(self):
        head = self.caches[0]
        return head._prev, head._flag

    def desc(self):
        pairs = [p for c in self.caches for p in c._pairs()]
        if len(pairs) > _lib.ROW_CACHE_MAX_PAIRS:
            raise ValueError(f"{self.what}: {len(pairs)} (table, stage) pairs, at most {_lib.ROW_CACHE_MAX_PAIRS} per select")
        key = tuple((t.data_ptr(), s.data_ptr()) for t, s in pairs)
        if self._desc[0] != key:
            arr = (_lib.RowPair * len(pairs))()
            for k, (t, s) in enumerate(pairs):
                if t.dtype != torch.float32 or s.dtype != torch.float32 or not t.is_contiguous() or not s.is_contiguous():
                    raise ValueError(f"{self.what}: tables and staged rows must be contiguous float32")
                width = s.numel()
                if t.numel() != t.shape[0] * width:
                    raise ValueError(f"{self.what}: a staged row of {width} against a table {tuple(t.shape)}")
                arr[k] = _lib.RowPair(t.data_ptr(), s.data_ptr(), width, t.shape[0])
            self._desc = (key, arr)
        return self._desc[1], len(pairs)

    def select(self, idx):
        head = self.caches[0]
        cell = _select_cell(idx, len(head.keys), head.table.device, self.what)
        prev, flag = self.cells()
        require_cuda(head.table, cell)
        arr, n = self.desc()
        check(_lib.lib().d3ga_row_cache_select(arr, n, dptr(cell), dptr(prev), dptr(flag), stream_handle()), "d3ga_row_cache_select")
        for c in self.caches:
            c._selected = True

    def flush(self):
        head = self.caches[0]
        if not any(c._selected for c in self.caches):
            return                                           # nothing was ever staged: the tables are the state
        prev, flag = self.cells()
        if not head.table.is_cuda:                           # a module moved to the CPU for a checkpoint: host bookkeeping
            p = int(prev)
            if p >= 0:
                for t, s in (p_ for c in self.caches for p_ in c._pairs()):
                    t[p] = s.detach().reshape(t[p].shape)
            return
        require_cuda(head.table)
        arr, n = self.desc()
        check(_lib.lib().d3ga_row_cache_flush(arr, n, dptr(prev), dptr(flag), stream_handle()), "d3ga_row_cache_flush")

    def check(self):
        if int(self.cells()[1]) != 0:
            raise IndexError(f"{self.what}: a select was given a row outside [0, {len(self.caches[0].keys)}): nothing was staged by "
                             "it, and the steps since then trained the row staged before")

    def unstage(self):
        """Write the staged rows back and forget them (before the tables are overwritten)."""
        self.flush()
        with torch.no_grad():
            self.cells()[0].fill_(-1)
        for c in self.caches:
            c._selected = False


class RowCache(nn.Module):
    """One nn.ParameterDict of (1,D) parameters (models/garment_net.py:104-106) as a table (N,D) plus ONE staged row.

    entries: an ordered {key: tensor (1,D)}.  The table is a buffer; `current` (1,D) is the only nn.Parameter: it is what the
    optimizer gets and what the forward reads.  `select(idx)` (an int, a key, or a (1,) int32 device cell) writes `current`
    back into the row it came from and stages row idx -- one launch, nothing when idx is the staged row.  A device cell
    outside [0, N) moves nothing and sets a sticky flag that `check()` turns into an IndexError.

    `select` must be called BEFORE the forward of a step: it overwrites `current` in place, behind autograd's back, and a
    tensor that autograd saved from `current` earlier in the step would change under it.  One staged row per cache: a batch of
    indices is a ValueError.

    `attach(optimizer)` lets the Adam state travel with the row (see there).  `state_dict()` flushes and emits the reference's
    layout, one `<key>` entry (1,D) per row, and `load_state_dict` reads it: `optimizable_poses.<seq>_<frame>` of a reference
    checkpoint loads with strict=True, and the other way round."""

    def __init__(self, entries, name="RowCache"):
        super().__init__()
        if len(entries) == 0:
            raise ValueError(f"{name}: no entries")
        self.keys = list(entries.keys())
        self._index = {k: i for i, k in enumerate(self.keys)}
        rows = [torch.as_tensor(v).detach().to(torch.float32).reshape(1, -1) for v in entries.values()]
        if any(r.shape != rows[0].shape for r in rows):
            raise ValueError(f"{name}: entries of different widths")
        self.name = name
        self.width = rows[0].shape[1]
        self.register_buffer("table", torch.cat(rows).contiguous(), persistent=False)
        self.register_buffer("_prev", torch.full((1,), -1, dtype=torch.int32), persistent=False)
        self.register_buffer("_flag", torch.zeros(1, dtype=torch.int32), persistent=False)
        self.current = nn.Parameter(torch.zeros(1, self.width))
        self._selected = False
        self._optimizer, self._opt_tables = None, None
        self.__dict__["_group"] = _Cells([self], name)

    def index(self, key):
        return self._index[key]

    def _pairs(self):
        pairs = [(self.table, self.current)]
        if self._optimizer is not None:
            st = self._optimizer.state[self.current]
            pairs += [(self._opt_tables[n], st[n]) for n in ("exp_avg", "exp_avg_sq", "step")]
        return pairs

    def select(self, idx):
        self._group.select(self._index[idx] if isinstance(idx, str) else idx)

    def flush(self):
        """Write the staged row (and its optimizer state) back into the tables; the row stays staged."""
        self._group.flush()

    def check(self):
        self._group.check()

    def attach(self, optimizer, tables=None):
        """Make the Adam state of `current` travel with the staged row: per-row tables exp_avg (N,D), exp_avg_sq (N,D), step (N,)
        are allocated (or taken from `tables`, see convert_optimizer_state) and added as pairs of the same select, and
        `optimizer.state[current]` is created in ClipAdam's layout if it is absent.  A row that is not selected keeps its moments
        and its own step count: the reference's lazy Adam over a ParameterDict, entry by entry.  Works with optim.ClipAdam and
        with torch.optim.Adam(capturable=True), whose `step` lives on the device; an Adam with a host `step` is refused.
        Call it outside a capture, and again after `optimizer.load_state_dict` (which replaces the state tensors)."""
        group = next((g for g in optimizer.param_groups if any(p is self.current for p in g["params"])), None)
        if group is None:
            raise ValueError(f"{self.name}.attach: `current` is not a parameter of this optimizer")
        from .optim import ClipAdam
        if not isinstance(optimizer, ClipAdam) and not (group.get("capturable") or group.get("fused")):
            raise ValueError(f"{self.name}.attach: this optimizer keeps `step` on the host, where a select cannot reach it; use "
                             "d3ga_amd.optim.ClipAdam or torch.optim.Adam(capturable=True)")
        require_cuda(self.current)
        dev = self.current.device
        st = optimizer.state[self.current]
        if len(st) == 0:
            st["step"] = torch.zeros((), dtype=torch.float32, device=dev)
            st["exp_avg"] = torch.zeros_like(self.current, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(self.current, memory_format=torch.contiguous_format)
        step = st["step"]
        if not (torch.is_tensor(step) and step.is_cuda and step.dtype == torch.float32 and step.numel() == 1):
            raise ValueError(f"{self.name}.attach: the optimizer's `step` must be a float32 device tensor")
        n = len(self.keys)
        given = tables is not None
        if not given:
            tables = {"exp_avg": torch.zeros(n, self.width), "exp_avg_sq": torch.zeros(n, self.width), "step": torch.zeros(n)}
        shapes = {"exp_avg": (n, self.width), "exp_avg_sq": (n, self.width), "step": (n,)}
        new = {}
        for k, shape in shapes.items():
            if tuple(tables[k].shape) != shape:
                raise ValueError(f"{self.name}.attach: table {k} is {tuple(tables[k].shape)}, expected {shape}")
            new[k] = tables[k].detach().to(device=dev, dtype=torch.float32).contiguous().clone()
        if given:
            self._group.unstage()                            # the tables are the state: whatever is staged goes back first
        else:
            self._group.flush()                              # (a row staged so far goes back without optimizer state)
        self._optimizer, self._opt_tables = optimizer, new

    def optimizer_tables(self):
        """The per-row optimizer state {exp_avg, exp_avg_sq, step} after a flush (None before attach)."""
        self.flush()
        return self._opt_tables

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        self._group.flush()
        for i, k in enumerate(self.keys):
            destination[prefix + k] = self.table[i:i + 1]

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        self._group.unstage()
        for i, k in enumerate(self.keys):
            v = state_dict.get(prefix + k)
            if v is None:
                missing_keys.append(prefix + k)
            elif tuple(v.shape) != (1, self.width):
                error_msgs.append(f"size mismatch for {prefix + k}: {tuple(v.shape)} in the checkpoint, (1, {self.width}) here")
            else:
                with torch.no_grad():
                    self.table[i].copy_(v.reshape(-1))
        if strict:
            unexpected_keys += [k for k in state_dict if k.startswith(prefix) and k[len(prefix):] not in self._index]


class FramePoses(nn.Module):
    """The three dictionaries of GarmentNet.prepare_opt_tensors (models/garment_net.py:87-107) over `assets["smplx"]`
    ({seq: {frame: {"Rh", "Th", "poses", ...}}}), keys f"{seq}_{str(frame).zfill(5)}": `optimizable_rotations` (3),
    `optimizable_translations` (3), `optimizable_poses` (87 or 165), each a RowCache.  ONE `select(idx)` / `flush()` serves the
    three and, after `attach(optimizer)`, their Adam state: 12 (table, stage) pairs in one launch.

    The reference re-creates its dictionaries inside the loop over sequences (lines 92-96), so with several sequences only the
    LAST one's frames exist there; this class registers all of them.  With one sequence (actorshq_actor02) the two agree.

    A model that must keep the reference's checkpoint keys takes the caches as its own attributes
    (`self.optimizable_poses = fp.optimizable_poses`, ...) and keeps `fp` out of its module tree (`self._fp = [fp]`)."""

    LRS = (("optimizable_rotations", 0.001), ("optimizable_translations", 0.0001), ("optimizable_poses", 0.001))

    def __init__(self, smplx):
        super().__init__()
        rot, trans, poses = OrderedDict(), OrderedDict(), OrderedDict()
        for seq in smplx.keys():
            for key, values in smplx[seq].items():
                k = f"{seq}_{str(key).zfill(5)}"
                rot[k] = torch.as_tensor(values["Rh"])[None]
                trans[k] = torch.as_tensor(values["Th"])[None]
                poses[k] = torch.as_tensor(values["poses"])[None]
        self.optimizable_rotations = RowCache(rot, "optimizable_rotations")
        self.optimizable_translations = RowCache(trans, "optimizable_translations")
        self.optimizable_poses = RowCache(poses, "optimizable_poses")
        self.keys = self.optimizable_poses.keys
        group = _Cells(self.caches, "FramePoses")
        self.__dict__["_group"] = group
        for c in self.caches:
            c.__dict__["_group"] = group

    @property
    def caches(self):
        return [self.optimizable_rotations, self.optimizable_translations, self.optimizable_poses]

    def index(self, key):
        return self.optimizable_poses.index(key)

    def select(self, idx):
        """Stage frame idx (an int, a key, or a (1,) int32 device cell) in the three caches; see RowCache for the rules."""
        self._group.select(self.index(idx) if isinstance(idx, str) else idx)

    def flush(self):
        self._group.flush()

    def check(self):
        self._group.check()

    def attach(self, optimizer, tables=None):
        """RowCache.attach for the three caches (tables: a list of three, as convert_optimizer_state returns them)."""
        for k, c in enumerate(self.caches):
            c.attach(optimizer, None if tables is None else tables[k])

    def get_parameters(self):
        """The reference's three learning-rate groups (models/garment_net.py:116-119), one staged parameter each."""
        return [{"params": [getattr(self, name).current], "lr": lr} for name, lr in self.LRS]

    def update(self, batch_smplx):
        """GarmentNet.update_batch (lines 220-232) for the staged frame: Rh, Th and poses of the batch become the three staged
        parameters, (1,D) each as the reference's entries are.  Returns poses."""
        batch_smplx["Rh"] = self.optimizable_rotations.current
        batch_smplx["Th"] = self.optimizable_translations.current
        batch_smplx["poses"] = self.optimizable_poses.current
        return batch_smplx["poses"]


# ---- optimizer checkpoints -------------------------------------------------------------------------------------------------
def convert_optimizer_state(state_dict, caches, to="tables", groups=None, tables=None):
    """Host only: an Adam `state_dict()` between the reference's layout and this module's.

    The optimizer entry of a reference checkpoint has N parameters in the group of every dictionary; the lazily stepped ones
    have state, the others none.  Here such a group has ONE parameter (`current`) and the per-row state lives in tables.
    caches: the RowCaches (or anything with `keys` and `width`) in group order; groups: the positions of their param groups
    (default 0, 1, ...: GarmentNet.get_parameters puts them first).

    to="tables":    -> (state_dict with one zero-state parameter per cache group, [ {exp_avg (N,D), exp_avg_sq (N,D), step (N,)} ]);
                    entries without state become zero rows with step 0.  Load the first into the optimizer and hand the tables
                    to `attach(optimizer, tables=...)`.
    to="reference": -> state_dict with N parameters per cache group, from `tables` (default: the caches' own after a flush);
                    a row with step 0 gets no state."""
    caches = list(caches)
    groups = list(range(len(caches))) if groups is None else list(groups)
    if to not in ("tables", "reference"):
        raise ValueError(f"convert_optimizer_state: to={to!r}, expected 'tables' or 'reference'")
    if to == "reference" and tables is None:
        tables = [c.optimizer_tables() for c in caches]
    state, out_state, out_groups, out_tables, at = state_dict["state"], {}, [], [], 0
    for gi, g in enumerate(state_dict["param_groups"]):
        ng = dict(g)
        ids = []
        if gi in groups:
            c = caches[groups.index(gi)]
            n, d = len(c.keys), c.width
            if to == "tables":
                if len(g["params"]) != n:
                    raise ValueError(f"convert_optimizer_state: group {gi} has {len(g['params'])} parameters, the cache {n} rows")
                t = {"exp_avg": torch.zeros(n, d), "exp_avg_sq": torch.zeros(n, d), "step": torch.zeros(n)}
                for r, pid in enumerate(g["params"]):
                    st = state.get(pid)
                    if st:
                        t["exp_avg"][r] = st["exp_avg"].detach().float().cpu().reshape(-1)
                        t["exp_avg_sq"][r] = st["exp_avg_sq"].detach().float().cpu().reshape(-1)
                        t["step"][r] = float(st["step"])
                out_tables.append(t)
                out_state[at] = {"step": torch.zeros(()), "exp_avg": torch.zeros(1, d), "exp_avg_sq": torch.zeros(1, d)}
                ids.append(at)
                at += 1
            else:
                if len(g["params"]) != 1:
                    raise ValueError(f"convert_optimizer_state: group {gi} has {len(g['params'])} parameters, expected the staged one")
                t = tables[groups.index(gi)]
                for r in range(n):
                    if float(t["step"][r]) > 0:
                        out_state[at] = {"step": t["step"][r].detach().float().cpu().reshape(()).clone(),
                                         "exp_avg": t["exp_avg"][r:r + 1].detach().float().cpu().clone(),
                                         "exp_avg_sq": t["exp_avg_sq"][r:r + 1].detach().float().cpu().clone()}
                    ids.append(at)
                    at += 1
        else:
            for pid in g["params"]:
                if pid in state:
                    out_state[at] = state[pid]
                ids.append(at)
                at += 1
        ng["params"] = ids
        out_groups.append(ng)
    out = {"state": out_state, "param_groups": out_groups}
    return (out, out_tables) if to == "tables" else out
