"""The training objective (csrc/objective.hip): the scale regulariser and the block of the reference's training
loop that turns the per-frame losses into the weighted total, with the NaN test left on the device.

Drop-ins for
    models/cage_net.py:226 (with :214)    scale_energy(scaling, delta_scale)
    train.py:190-244                      TrainingObjective(...)(frames)
    train.py:64-69   check_loss           objective.poll() after every step / replay, objective.check() when it may wait
    train.py:50-61   stringify            objective.report()
GPU tensors only.  Everything is capturable inside `graph.CapturedStep`: no call here reads a device value on the host except
`check()` and `report()`.

    objective = TrainingObjective.from_config(config.train)
    def step():
        ...
        total = objective(frames)          # frames: one dict per frame of the batch (keys: TrainingObjective.KEYS)
        total.backward()
        opt.step()
    cap = CapturedStep(step, params=params, slots=...)
    for it in range(n):
        cap.replay(...)
        objective.poll()                   # raises ValueError("loss is NaN ...") once a copy with the flag has arrived
        if it % log_n_steps == 0:
            progress_bar.set_postfix(objective.report())
"""
import torch

from . import _lib
from ._lib import check, dptr, f32c16, stream_handle

__all__ = ["scale_energy", "TrainingObjective"]

_ACTIVATIONS = {"exp": _lib.SCALE_ACT_EXP, "none": _lib.SCALE_ACT_NONE, None: _lib.SCALE_ACT_NONE}


def _on_gpu(what, *tensors):
    """ValueError for anything that is not a tensor on the current GPU (there is no CPU fallback)."""
    cur = None
    for t in tensors:
        if t is None:
            continue
        if not torch.is_tensor(t):
            raise ValueError(f"{what}: expected a tensor, got {type(t).__name__}")
        if not t.is_cuda:
            raise ValueError(f"{what}: runs on the GPU only (tensor on {t.device}); there is no CPU fallback")
        if cur is None:
            cur = torch.cuda.current_device()
        if t.device.index != cur:
            raise ValueError(f"{what}: tensor on {t.device} but the current device is cuda:{cur} (launches go to the current "
                             f"device's stream)")


class _ScaleEnergy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scaling, delta, act):
        a, b = f32c16(scaling), f32c16(delta)
        n = a.numel()
        # [0]: the energy; [4:]: one partial sum per workgroup (two-stage reduction: no zero fill, no atomics, reproducible)
        buf = torch.empty(4 + _lib.LOSS_PARTIALS, dtype=torch.float32, device=a.device)
        out = buf[:1]
        check(_lib.lib().d3ga_scale_energy_fwd(n, dptr(a), dptr(b), act, dptr(out), dptr(buf[4:]), stream_handle()),
              "d3ga_scale_energy_fwd")
        ctx.save_for_backward(*([a] if b is None else [a, b]))       # the inputs themselves: nothing of size (P,3) is made
        ctx.act = act
        return out

    @staticmethod
    def backward(ctx, g):
        a = ctx.saved_tensors[0]
        b = ctx.saved_tensors[1] if len(ctx.saved_tensors) > 1 else None
        need_a, need_b = ctx.needs_input_grad[0], b is not None and ctx.needs_input_grad[1]
        if not (need_a or need_b):
            return None, None, None
        grad = torch.empty_like(a)                                   # written once; both inputs receive it
        check(_lib.lib().d3ga_scale_energy_bwd(a.numel(), dptr(a), dptr(b), ctx.act, dptr(f32c16(g)), dptr(grad), stream_handle()),
              "d3ga_scale_energy_bwd")
        return (grad if need_a else None), (grad if need_b else None), None


def scale_energy(scaling, delta_scale=None, activation="exp"):
    """th.mean(th.mean(act(scaling + delta_scale)**2, axis=1))[None] (models/cage_net.py:214, 226) -> (1,) float32.

    scaling: (P,3) (any shape with rows of equal length: the mean of the row means is the mean of all elements);
    delta_scale: the same shape, or None.  activation: "exp" (both networks of the reference) or "none" (squares the sum as it
    is).  The activated scales are never written: the forward reads the two inputs once and adds the squares in two stages
    of a fixed order (no atomics: two calls, and a graph replay, are equal bit for bit); the backward recomputes the
    activation and writes ONE (P,3) array, g * 2 act(x) act'(x) / (3P), which both inputs receive -- only the ones that require
    a gradient.  Saved for the backward: the inputs themselves.

    Alignment: the kernels load 16 bytes per lane over the flat array and handle the tail of 3P mod 4 floats themselves; an
    input that is not float32, not contiguous, or a view whose storage offset leaves it off a 16-byte boundary goes through
    `_lib.f32c16` (one copy) as in the other operators -- the kernels do not handle a misaligned base."""
    if activation not in _ACTIVATIONS:
        raise ValueError(f"scale_energy: activation={activation!r}, expected 'exp' or 'none'")
    if delta_scale is not None and delta_scale.shape != scaling.shape:
        raise ValueError(f"scale_energy: scaling {tuple(scaling.shape)} and delta_scale {tuple(delta_scale.shape)} differ")
    if scaling.numel() == 0:
        raise ValueError("scale_energy: no elements")
    _on_gpu("scale_energy", scaling, delta_scale)
    return _ScaleEnergy.apply(scaling, delta_scale, _ACTIVATIONS[activation])


class _Objective(torch.autograd.Function):
    @staticmethod
    def forward(ctx, owner, n_frames, layout, *tensors):
        # layout: per tensor (frame, slot); tensors: flat contiguous float32
        desc = owner._desc(n_frames, layout, tensors, None)
        out = torch.empty(1 + _lib.OBJ_TERMS, dtype=torch.float32, device=tensors[0].device)
        check(_lib.lib().d3ga_objective_fwd(desc, dptr(out), dptr(owner._cell(out.device)), stream_handle()), "d3ga_objective_fwd")
        ctx.owner, ctx.n_frames, ctx.layout = owner, n_frames, layout
        ctx.save_for_backward(*tensors)
        total, terms = out[0], out[1:]
        ctx.mark_non_differentiable(terms)
        return total, terms

    @staticmethod
    def backward(ctx, g, _g_terms):
        tensors = ctx.saved_tensors
        need = ctx.needs_input_grad[3:]
        offsets, at = [], 0
        for t, nd in zip(tensors, need):
            offsets.append(at if nd else -1)
            at += t.numel() if nd else 0
        if at == 0:
            return (None,) * (3 + len(tensors))
        desc = ctx.owner._desc(ctx.n_frames, ctx.layout, tensors, offsets)
        grads = torch.empty(at, dtype=torch.float32, device=g.device)      # every element is written by the one launch
        check(_lib.lib().d3ga_objective_bwd(desc, dptr(g.float().contiguous()), dptr(grads), at, stream_handle()), "d3ga_objective_bwd")
        return (None, None, None) + tuple(None if o < 0 else grads[o:o + t.numel()].view(t.shape) for t, o in zip(tensors, offsets))


class TrainingObjective:
    """train.py:190-244 as one launch each way: the weighted total of a batch of frames, its nine terms, and the NaN flag.

    objective(frames) -> total (0-d, differentiable in every input that requires a gradient).  frames: a list of 1..16 dicts,
    one per frame, all device tensors, none read on the host:
        l1, ssim            0-d (what losses.l1_ssim returns)          sil_l1            0-d
        scale_energy        (n_cages,)                                 fm_energy         (n_cages,) or None
        frame_encoding      (D,), required                             optimizable_poses (1,N) or None
        blur_weights        (1,3) or None                              vgg               0-d or None
    Every frame must have the same optional entries and the same n_cages; at most 4096 elements per entry.  A missing
    `frame_encoding`, frames that differ, or a tensor that is not on the GPU raise ValueError before anything is launched.

    With B frames (objective_math.h holds the arithmetic and its fixed summation orders):
        color_loss = mean_f((1-l) l1_f + l (1 - ssim_f)) rgb_weight        sil_loss = mean_f(sil_l1_f) sil_weight
        codes_reg  = mean_f(0.001 mean(enc_f^2) [+ 0.0075 mean(poses_f^2)])   scale_loss = mean over (B, n_cages) of 175 scale_energy
        fme_loss   = mean_f(mean(fm_energy_f) + 3) fme_weight               blur_loss = mean_f(mean|blur_weights_f - 1|) blur_weight
        vgg_loss   = mean_f(vgg_f) vgg_weight                               bg_loss = 0 (the reference never appends to it)
        total_loss = color + sil + bg + codes + scale + fme + blur + vgg    (an absent optional entry: its term is 0)

    `terms` (after a call): the nine float32 values on the device, in the reference's key order (KEY_ORDER).
    The status cell {nan_seen, first_bad_step, steps} lives on the device and is updated by the forward kernel: `steps` counts
    the calls (and the replays of a captured one); the first NaN total (NaN only, as th.isnan: an infinite total is not
    flagged) records its step and keeps that step's terms.  `check()`, `poll()`, `report()`, `status()` read it."""

    KEYS = ("l1", "ssim", "sil_l1", "scale_energy", "fm_energy", "frame_encoding", "optimizable_poses", "blur_weights", "vgg")
    OPTIONAL = ("fm_energy", "optimizable_poses", "blur_weights", "vgg")
    SCALARS = ("l1", "ssim", "sil_l1", "vgg")
    KEY_ORDER = ("color_loss", "sil_loss", "scale_loss", "fme_loss", "blur_loss", "vgg_loss", "bg_loss", "codes_reg", "total_loss")

    def __init__(self, lambda_dssim, rgb_weight, sil_weight, fme_weight, blur_weight, vgg_weight, first_iteration=1):
        """first_iteration: the loop counter of the first call (train.py:112 starts at 1), for the `iter=` of the error message"""
        self.weights = tuple(float(w) for w in (lambda_dssim, rgb_weight, sil_weight, fme_weight, blur_weight, vgg_weight))
        self.first_iteration = int(first_iteration)
        self.terms = None
        self._status = None
        self._descs = {}
        self._host, self._event = None, None

    @classmethod
    def from_config(cls, train, **kwargs):
        """train: `config.train` of the reference (attributes or keys lambda_dssim, rgb_weight, sil_weight, fme_weight,
        blur_weight, vgg_weight; shadow_weight and bg_weight are read by train.py and never used)"""
        get = (lambda k: train[k]) if isinstance(train, dict) else (lambda k: getattr(train, k))
        return cls(*[get(k) for k in ("lambda_dssim", "rgb_weight", "sil_weight", "fme_weight", "blur_weight", "vgg_weight")], **kwargs)

    # ---- the call --------------------------------------------------------------------------------------------------------------
    def _gather(self, frames):
        """(layout, tensors) of a checked batch: per tensor its (frame, slot), flat contiguous float32"""
        if not isinstance(frames, (list, tuple)) or not 1 <= len(frames) <= _lib.OBJ_MAX_FRAMES:
            raise ValueError(f"TrainingObjective: expected a list of 1..{_lib.OBJ_MAX_FRAMES} frame dicts")
        present = None
        for f, fr in enumerate(frames):
            if fr.get("frame_encoding") is None:
                raise ValueError(f"TrainingObjective: frame {f} has no frame_encoding (train.py:195 fails on it too)")
            for k in self.KEYS:
                if k not in self.OPTIONAL and fr.get(k) is None:
                    raise ValueError(f"TrainingObjective: frame {f} has no {k}")
            have = tuple(k for k in self.OPTIONAL if fr.get(k) is not None)
            if present is None:
                present = have
            elif have != present:
                raise ValueError(f"TrainingObjective: frame {f} has the optional entries {have}, frame 0 has {present}: every frame "
                                 "of a batch must have the same ones")
        layout, tensors = [], []
        for f, fr in enumerate(frames):
            for slot, k in enumerate(self.KEYS):
                t = fr.get(k)
                if t is None:
                    continue
                if not torch.is_tensor(t):
                    raise ValueError(f"TrainingObjective: frame {f} {k}: expected a tensor, got {type(t).__name__}")
                n = t.numel()
                if k in self.SCALARS and n != 1:
                    raise ValueError(f"TrainingObjective: frame {f} {k}: expected one element, got {tuple(t.shape)}")
                if not 1 <= n <= _lib.OBJ_MAX_LEN:
                    raise ValueError(f"TrainingObjective: frame {f} {k}: {n} elements, expected 1..{_lib.OBJ_MAX_LEN}")
                if k in ("scale_energy", "fm_energy") and n != frames[0][k].numel():
                    raise ValueError(f"TrainingObjective: frame {f} {k} has {n} cages, frame 0 has {frames[0][k].numel()}")
                layout.append((f, slot))
                tensors.append(t)
        _on_gpu("TrainingObjective", *tensors)
        tensors = [t.float().contiguous().reshape(-1) for t in tensors]
        return tuple(layout), tensors

    def _desc(self, n_frames, layout, tensors, offsets):
        """struct d3ga_objective_desc of an input signature (addresses, lengths, gradient offsets), built once per signature"""
        key = (n_frames, layout, tuple(t.data_ptr() for t in tensors), tuple(t.numel() for t in tensors),
               None if offsets is None else tuple(offsets), self.weights)
        d = self._descs.get(key)
        if d is None:
            if len(self._descs) >= 64:
                self._descs.clear()
            d = _lib.ObjectiveDesc()
            d.n_frames = n_frames
            (d.lambda_dssim, d.rgb_weight, d.sil_weight, d.fme_weight, d.blur_weight, d.vgg_weight) = self.weights
            for i, ((f, slot), t) in enumerate(zip(layout, tensors)):
                e = d.entry[f * _lib.OBJ_SLOTS + slot]
                e.ptr, e.len, e.goff = t.data_ptr(), t.numel(), -1 if offsets is None else offsets[i]
            self._descs[key] = d
        return d

    def _cell(self, device):
        if self._status is None or self._status.device != device:
            self._status = torch.zeros(_lib.OBJ_STATUS_WORDS, dtype=torch.int32, device=device)
            self._host, self._event = None, None
        return self._status

    def __call__(self, frames):
        layout, tensors = self._gather(frames)
        total, self.terms = _Objective.apply(self, len(frames), layout, *tensors)
        return total

    # ---- the status cell ---------------------------------------------------------------------------------------------------
    def _losses(self, values):
        return {k: float(v) for k, v in zip(self.KEY_ORDER, values)}

    def _raise_if_bad(self, words):
        """words: the 16 status words on the host"""
        if int(words[_lib.OBJ_STATUS_NAN_SEEN]) == 0:
            return
        step = int(words[_lib.OBJ_STATUS_FIRST_BAD])
        bad = words[_lib.OBJ_STATUS_TERMS:_lib.OBJ_STATUS_TERMS + _lib.OBJ_TERMS].view(torch.float32).tolist()
        loss_str = " ".join(f"{k}={v:.5f}" for k, v in self._losses(bad).items())          # train.py:50-61, 67
        raise ValueError(f"loss is NaN: iter={self.first_iteration + step}: {loss_str}")

    def status(self):
        """{nan_seen, first_bad_step, steps} read synchronously (first_bad_step: 0-based call number, None without a NaN)"""
        if self._status is None:
            return {"nan_seen": False, "first_bad_step": None, "steps": 0}
        w = self._status.cpu()
        seen = bool(int(w[_lib.OBJ_STATUS_NAN_SEEN]))
        return {"nan_seen": seen, "first_bad_step": int(w[_lib.OBJ_STATUS_FIRST_BAD]) if seen else None,
                "steps": int(w[_lib.OBJ_STATUS_STEPS])}

    def check(self):
        """check_loss (train.py:64-69), synchronously: raises ValueError("loss is NaN: iter=... color_loss=... ...") with the nine
        terms of the FIRST step whose total was NaN.  The flag is sticky: later finite steps do not clear it."""
        if self._status is not None:
            self._raise_if_bad(self._status.cpu())

    def poll(self):
        """The same without ever waiting (as graph._OverflowWatch): looks at the last asynchronous copy of the status words if
        it has arrived, and raises then; otherwise starts a copy to pinned memory behind the work enqueued so far.  Call it
        after every step or replay: a NaN is reported within two calls of the copy's arrival."""
        if self._status is None:
            return
        if self._event is not None:
            if not self._event.query():
                return
            self._event = None
            self._raise_if_bad(self._host)
        if self._host is None:
            self._host = torch.zeros(_lib.OBJ_STATUS_WORDS, dtype=torch.int32).pin_memory()
        self._host.copy_(self._status, non_blocking=True)
        self._event = torch.cuda.Event()
        self._event.record()

    def report(self):
        """The reference's `losses` dict (train.py:246-256) of the last call or replay as Python floats, in key order, from ONE
        read-back -- for progress_bar.set_postfix / tb_writer in place of stringify's nine .item() calls."""
        if self.terms is None:
            raise ValueError("TrainingObjective.report: the objective has not been called")
        return self._losses(self.terms.tolist())
