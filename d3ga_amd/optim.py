"""Gradient clipping + Adam for all parameters of a model in three HIP launches (csrc/optim.hip).

Drop-in for the tail of the reference's training iteration (models/trainer.py:186-192)

    loss.backward()
    th.nn.utils.clip_grad_norm_(self.model.parameters(), 2.5, foreach=True)      # <- goes away
    self.optimizer.step()                                                         # <- ClipAdam(..., max_norm=2.5)
    self.scheduler.step()
    self.optimizer.zero_grad()

with `torch.optim.Adam`'s arithmetic, state layout (`state[p] = {"step", "exp_avg", "exp_avg_sq"}`) and checkpoint format:
`state_dict()` loads into `torch.optim.Adam` and the other way round.  `step` is a 0-dim float32 tensor ON THE DEVICE (where
torch's `capturable=True` keeps it), which the kernels increment themselves, so `step()` can be captured by `graph.CapturedStep`.

    opt = ClipAdam(model.get_parameters(), lr=1e-3, max_norm=2.5)                 # max_norm=None: plain Adam
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[200_000, 350_000, 500_000], gamma=0.33)
    loss.backward(); opt.step(); sched.step(); opt.zero_grad()
    opt.grad_norm                                    # 0-dim device tensor: what clip_grad_norm_ returned

What differs from the two torch calls:
  * the norm runs over the parameters of THIS optimizer's groups that have a gradient (the reference's runs over
    `model.parameters()`): the same whenever every trained parameter is in a group;
  * `.grad` is left UNCLIPPED (the clip coefficient is applied inside the update; the reference zeroes the gradients in the
    next line anyway);
  * a parameter whose `.grad` is None takes no part, as in torch: not in the norm, no moment decay, its `step` stays.
Inside a captured step the learning rates are read from a small device array: call `opt.flush_hyperparams()` after
`sched.step()` (one small asynchronous copy when something changed).  An eager `step()` does that itself.  Keep the optimizer
alive as long as a graph that contains its step is replayed; after `add_param_group` such a graph must be captured again.
The optimizer holds no reference to the gradients between steps: `zero_grad()` frees them, and as long as the next backward
gets the same addresses (what the caching allocator does in a steady loop) nothing is rebuilt or uploaded (`plan_uploads`).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import D3GAError, check, require_cuda, stream_handle

# struct d3ga_optim_chunk / d3ga_optim_tensor (include/d3ga.h)
CHUNK_DTYPE = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i4"), ("tensor", "<i4"), ("flags", "<i4"),
                        ("reserved", "<i4")])
TENSOR_DTYPE = np.dtype([("step", "<u8"), ("group", "<i4"), ("reserved", "<i4")])
assert CHUNK_DTYPE.itemsize == 48 and TENSOR_DTYPE.itemsize == 16


def n_chunks_of(numel, chunk=_lib.OPTIM_CHUNK):
    return (int(numel) + chunk - 1) // chunk


def plan_key(live):
    """live: one (p_ptr, g_ptr, numel, group) per parameter that has a gradient, in group order.  Two steps with equal keys use the
    same tables."""
    return tuple((int(a), int(b), int(n), int(k)) for a, b, n, k in live)


def build_plan(entries, chunk=_lib.OPTIM_CHUNK):
    """entries: one (p_ptr, g_ptr, m_ptr, v_ptr, numel, step_ptr, group) per tensor (numel >= 1) -> (chunk table, tensor table)
    as numpy records laid out like the C structs.  A tensor of n elements becomes ceil(n / chunk) consecutive records, the last
    one with the n % chunk elements that remain; a chunk is flagged OPTIM_ALIGNED16 when its four addresses are multiples of 16
    (`chunk` is a multiple of 4, so all chunks of a tensor agree)."""
    counts = [n_chunks_of(e[4], chunk) for e in entries]
    table = np.zeros(sum(counts), dtype=CHUNK_DTYPE)
    tensors = np.zeros(len(entries), dtype=TENSOR_DTYPE)
    at = 0
    for t, ((p, g, m, v, numel, step, group), k) in enumerate(zip(entries, counts)):
        if numel < 1:
            raise ValueError("build_plan: empty tensor")
        rows = table[at:at + k]
        off = np.arange(k, dtype=np.uint64) * np.uint64(4 * chunk)
        rows["p"], rows["g"], rows["m"], rows["v"] = np.uint64(p) + off, np.uint64(g) + off, np.uint64(m) + off, np.uint64(v) + off
        rows["n"] = chunk
        rows["n"][-1] = numel - (k - 1) * chunk
        rows["tensor"] = t
        rows["flags"] = _lib.OPTIM_ALIGNED16 if (p | g | m | v) % 16 == 0 else 0
        tensors[t] = (step, group, 0)
        at += k
    return table, tensors


class _PinnedRing:
    """Pinned host buffers used in turn for asynchronous uploads: a buffer is rewritten only after the copy that last read it
    has run (zero_grad(set_to_none=True) moves the gradients, so an eager loop may upload a new plan every step)."""

    def __init__(self, nbytes, n=2):
        self.bufs = [torch.empty(nbytes, dtype=torch.uint8).pin_memory() for _ in range(n)]
        self.events, self.at = [None] * n, 0

    def take(self):
        i = self.at
        self.at = (i + 1) % len(self.bufs)
        if self.events[i] is not None:
            self.events[i].synchronize()
        return i, self.bufs[i]

    def sent(self, i):
        self.events[i] = torch.cuda.Event()
        self.events[i].record()


class ClipAdam(torch.optim.Optimizer):
    """clip_grad_norm_(params, max_norm) + torch.optim.Adam in three launches; see the module docstring.  Keyword arguments are
    `torch.optim.Adam`'s (utils/load_module.py:20-26 calls `cls(**config, params=params)`) plus `max_norm`.  What the reference
    does not use is refused: amsgrad, maximize, weight_decay, differentiable."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, max_norm=None,
                 maximize=False, differentiable=False, foreach=None, capturable=False, fused=None):
        if max_norm is not None and not float(max_norm) >= 0.0:
            raise ValueError(f"ClipAdam: max_norm must be None or >= 0, got {max_norm}")
        self.max_norm = None if max_norm is None else float(max_norm)
        self.grad_norm = None              # 0-dim device tensor once a clipped step has been issued
        self._device = None
        self._plan_key = None
        self._buffers_for = None
        self._hp_uploaded = None
        self.plan_uploads = 0              # times the tables were rebuilt (eager: + uploaded); stays put while no address moves
        self._captured = []                # pinned tables of plans built under capture: read by every replay
        # foreach / fused / capturable choose between torch's implementations and mean nothing here; the groups carry torch's
        # defaults so that a state_dict looks like Adam's.  capturable=False on purpose: a torch.optim.Adam that loads this
        # state then forms its bias corrections on the host in double, as the reference's optimizer does (its capturable path
        # forms them in float32 on the device: 1 - 0.999^t loses five digits for small t).
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=None,
                        capturable=False, differentiable=differentiable, fused=None)
        super().__init__(params, defaults)

    # ---- what is accepted --------------------------------------------------------------------------------
    @staticmethod
    def _check_options(group):
        if group.get("amsgrad"):
            raise ValueError("ClipAdam: amsgrad=True is not supported")
        if group.get("maximize"):
            raise ValueError("ClipAdam: maximize=True is not supported")
        if group.get("weight_decay", 0) != 0:
            raise ValueError(f"ClipAdam: weight_decay={group['weight_decay']} is not supported (must be 0)")
        if group.get("differentiable"):
            raise ValueError("ClipAdam: differentiable=True is not supported")
        lr, (b1, b2), eps = group["lr"], group["betas"], group["eps"]
        if torch.is_tensor(lr) or not float(lr) >= 0.0:
            raise ValueError(f"ClipAdam: lr must be a non-negative number, got {lr}")
        if not 0.0 <= float(b1) < 1.0 or not 0.0 <= float(b2) < 1.0:
            raise ValueError(f"ClipAdam: betas must lie in [0, 1), got {group['betas']}")
        if not float(eps) >= 0.0:
            raise ValueError(f"ClipAdam: eps must be >= 0, got {eps}")

    def add_param_group(self, param_group):
        """As torch's.  The device buffers are allocated anew by the next (eager) step: a graph captured before the call still
        points at the old ones and must be captured again."""
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        try:
            self._check_options(group)
            for p in group["params"]:
                if p.dtype != torch.float32:
                    raise ValueError(f"ClipAdam: params must be float32, got {p.dtype}")
                if p.layout != torch.strided or not p.is_contiguous():
                    raise ValueError(f"ClipAdam: params must be dense and contiguous, got a {tuple(p.shape)} tensor with strides {p.stride() if p.layout == torch.strided else p.layout}")
                if self._device is None:
                    self._device = p.device
                if p.device != self._device:
                    raise ValueError(f"ClipAdam: params on more than one device ({self._device} and {p.device})")
            if self._device is not None and self._device.type != "cuda":
                raise D3GAError(f"ClipAdam runs on the GPU only (params on {self._device}); there is no CPU fallback")
        except Exception:
            self.param_groups.pop()
            if not self.param_groups:
                self._device = None
            raise
        self._buffers_for = None

    # ---- device-side state -------------------------------------------------------------------------------
    def _ensure_buffers(self, capturing):
        """Device tables, scratch and staging sized for EVERY parameter having a gradient; allocated outside a capture."""
        sig = (len(self.param_groups), sum(len(g["params"]) for g in self.param_groups))
        if self._buffers_for == sig:
            return
        if capturing:
            raise RuntimeError("ClipAdam: the first step() (and the first one after add_param_group) must run eagerly: it allocates")
        n_t = max(sig[1], 1)
        n_c = max(sum(n_chunks_of(p.numel()) for g in self.param_groups for p in g["params"]), 1)
        dev = self._device
        self._tensor_off = (48 * n_c + 255) // 256 * 256
        self._table_bytes = self._tensor_off + 16 * n_t
        self._tables = torch.empty(self._table_bytes, dtype=torch.uint8, device=dev)
        need = ctypes.c_int64()
        check(_lib.lib().d3ga_optim_scratch_bytes(n_c, n_t, sig[0], ctypes.byref(need)), "d3ga_optim_scratch_bytes")
        self._scratch = torch.empty(need.value, dtype=torch.uint8, device=dev)
        self._hp = torch.zeros(4 * sig[0], dtype=torch.float64, device=dev)
        self._hp_ring = _PinnedRing(32 * sig[0])
        self._ring = _PinnedRing(self._table_bytes)
        self._spare = None
        if self.grad_norm is None:
            self.grad_norm = torch.zeros((), dtype=torch.float32, device=dev)
        self._hp_uploaded = None
        self._plan_key = None
        self._buffers_for = sig

    def _pin_spare(self):
        """The pinned table buffer of the next captured step, made ready outside a capture."""
        if self._spare is None and self._buffers_for is not None:
            self._spare = torch.empty(self._table_bytes, dtype=torch.uint8).pin_memory()

    def flush_hyperparams(self):
        """Carry lr / betas / eps of the groups to the device array the kernels read, if they differ from what is there.  An eager
        step() calls this itself; around a captured step call it after `scheduler.step()`."""
        vals = tuple((float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"])) for g in self.param_groups)
        capturing = torch.cuda.is_current_stream_capturing()
        if not capturing:
            self._pin_spare()                  # (a capture consumed the last one)
        if vals == self._hp_uploaded:
            return
        self._ensure_buffers(capturing)
        if capturing:
            raise RuntimeError("ClipAdam: hyperparameters changed inside a capture; call flush_hyperparams() outside of it "
                               "(a captured copy would put the OLD values back on every replay)")
        for g in self.param_groups:
            self._check_options(g)
        i, buf = self._hp_ring.take()
        host = buf.view(torch.float64)
        host.copy_(torch.tensor(vals, dtype=torch.float64).reshape(-1))
        self._hp.copy_(host, non_blocking=True)
        self._hp_ring.sent(i)
        self._hp_uploaded = vals

    def _upload_plan(self, entries, capturing):
        table, tensors = build_plan(entries)
        nbytes = self._tensor_off + tensors.nbytes
        if capturing:
            # No copy is captured: the kernels of a captured step read their tables from pinned host memory (mapped to the
            # device), once per replay.  That buffer belongs to this plan alone and is kept, never rewritten, for the optimizer's
            # lifetime -- keep the optimizer alive as long as the graph is replayed.  It was pinned before the capture began
            # (pinning allocates).
            stage, self._spare = self._spare, None
            if stage is None:
                raise RuntimeError("ClipAdam: a second capture without an eager step() or flush_hyperparams() in between: the pinned "
                                   "table of a captured step is prepared by those (pinning allocates, which a capture cannot)")
        else:
            i, stage = self._ring.take()
        self.plan_uploads += 1
        host = stage.numpy()
        host[:table.nbytes] = table.view(np.uint8).reshape(-1)
        host[self._tensor_off:nbytes] = tensors.view(np.uint8).reshape(-1)
        if capturing:
            self._captured.append(stage)
            return stage.data_ptr(), len(table), len(tensors)
        self._tables[:nbytes].copy_(stage[:nbytes], non_blocking=True)
        self._ring.sent(i)
        return self._tables.data_ptr(), len(table), len(tensors)

    # ---- the step ----------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        capturing = torch.cuda.is_current_stream_capturing()
        live, tensors = [], []
        for k, group in enumerate(self.param_groups):
            for p in group["params"]:
                g = p.grad
                if g is None or p.numel() == 0:
                    continue
                if g.is_sparse:
                    raise ValueError("ClipAdam: sparse gradients are not supported")
                if g.dtype != torch.float32 or g.device != p.device:
                    raise ValueError(f"ClipAdam: gradient is {g.dtype} on {g.device}, expected float32 on {p.device}")
                if not g.is_contiguous():
                    if capturing:
                        raise ValueError("ClipAdam: non-contiguous gradient inside a capture (the contiguous copy would not be the "
                                         "tensor later replays write)")
                    g = g.contiguous()
                st = self.state[p]
                if len(st) == 0:
                    if capturing:
                        raise RuntimeError("ClipAdam: optimizer state would be created inside a capture; run one eager step first")
                    st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                live.append((p.data_ptr(), g.data_ptr(), p.numel(), k))
                tensors.append((p, g, st))
        if not live:
            return loss
        require_cuda(tensors[0][0])
        self._ensure_buffers(capturing)
        self.flush_hyperparams()
        key = plan_key(live)
        if capturing or key != self._plan_key:         # (a captured step never shares tables with eager steps, which rewrite theirs)
            entries = [(p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel(),
                        st["step"].data_ptr(), k) for (p, g, st), (_, _, _, k) in zip(tensors, live)]
            self._plan = self._upload_plan(entries, capturing)
            # (capturing executes nothing: the tables of a plan built there are not on the device until a replay has run)
            self._plan_key = None if capturing else key
        if not capturing:
            self._pin_spare()
        base, n_chunks, n_tensors = self._plan
        check(_lib.lib().d3ga_optim_clip_adam_step(
            ctypes.c_void_p(base), n_chunks, ctypes.c_void_p(base + self._tensor_off), n_tensors, ctypes.c_void_p(self._hp.data_ptr()),
            len(self.param_groups), -1.0 if self.max_norm is None else self.max_norm, ctypes.c_void_p(self._scratch.data_ptr()),
            ctypes.c_void_p(self.grad_norm.data_ptr()), stream_handle()), "d3ga_optim_clip_adam_step")
        return loss

    # ---- checkpoints -------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict):
        """Accepts `torch.optim.Adam`'s state_dict (a reference checkpoint's optimizer entry): `step` as a number, a CPU tensor or
        a device tensor."""
        super().load_state_dict(state_dict)
        for g in self.param_groups:
            self._check_options(g)
        for p, st in self.state.items():
            if len(st) == 0:
                continue
            step = st["step"]
            step = step.detach().to(device=p.device, dtype=torch.float32).reshape(()).clone() if torch.is_tensor(step) else \
                torch.tensor(float(step), dtype=torch.float32, device=p.device)
            st["step"] = step
            for name in ("exp_avg", "exp_avg_sq"):
                st[name] = st[name].detach().to(device=p.device, dtype=torch.float32).contiguous()
        self._plan_key = None
        self._hp_uploaded = None
