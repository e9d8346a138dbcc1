"""Differentiable tile rasterizer with the operator surface of `diff_gaussian_rasterization` (branch dr_aa).

Mirrors what renderer.py:13-16,79-93,130-141 of the reference imports and calls:
    GaussianRasterizationSettings(image_height, image_width, tanfovx, tanfovy, bg, scale_modifier, viewmatrix,
                                  projmatrix, sh_degree, campos, prefiltered, debug, antialiasing)
    GaussianRasterizer(raster_settings)(means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None,
                                        rotations=None, cov3D_precomp=None) -> (color (3,H,W), radii (P,), invdepth (1,H,W))
backed by the gfx950 kernels of libd3ga_hip.so (include/d3ga.h).  GPU tensors only, no CPU fallback.

Scratch ("geomBuffer / binningBuffer / imgBuffer") is allocated from torch's caching allocator per call and kept
alive in the autograd context.  The duplicate capacity of the binning lists is a per-device high-water mark; after
the forward has been enqueued the 16-byte counter block is read back (the only host sync, the analogue of upstream
reading `num_rendered`) and the call is repeated with a larger buffer in the rare case of overflow.  With
``set_capacity_policy("static", n)`` nothing is read back (graph-capturable; caller checks `last_counters()`).
"""
import ctypes
import os
from typing import NamedTuple, Optional

import torch
from torch import nn

from . import _lib
from ._lib import RasterParams, check, dptr, require_cuda, stream_handle


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool
    antialiasing: bool = False
    # extension (not in upstream): bin every Gaussian by its alpha >= 1/255 box instead of the reference's 3-sigma square
    # (d3ga_raster_params::tile_cull).  Off: tile lists, D and max_tile are upstream's.  On: the same image bit for bit from
    # shorter lists -- every tile's list a subsequence of upstream's.  renderer.render / render_l1 / render_pair turn it on.
    tile_cull: bool = False


# ------------------------------------------------------------------------------------------------------------
# capacity policy for the binning lists
# ------------------------------------------------------------------------------------------------------------
_policy = {"mode": "auto", "static": 0}
_hwm = {}            # device index -> high-water mark of D
_last = {}           # device index -> (binning tensor, capacity) of the most recent forward (for last_counters)
_last_img = {}       # device index -> (img scratch tensor, W, H) of the most recent forward (for last_termination)
_capture_log = None  # while graph.CapturedStep / CapturedCutStep capture: list of (binning tensor, capacity) of EVERY forward issued


def set_capacity_policy(mode, capacity=0):
    """"auto": read the duplicate count back after every forward and retry on overflow (default).
    "static": use `capacity` duplicates, never synchronise; check `last_counters()["overflow"]` yourself.  A view-batched
    render (raster_views) bins its k views into ONE list, so a static capacity counts the duplicates of all k views together."""
    if mode not in ("auto", "static"):
        raise ValueError(mode)
    _policy["mode"] = mode
    _policy["static"] = int(capacity)


def _record_forward(dev, binning, cap):
    _last[dev.index] = (binning, cap)
    if _capture_log is not None:
        _capture_log.append((binning, cap))


def _forward_with_capacity(P, k, dev, launch):
    """The capacity policy around one forward of k views (k = 1: the single-view operator).  launch(cap) -> (geom, binning, img)
    enqueues the forward with room for `cap` duplicates; "auto" reads the counter block back (the only host sync, upstream:
    num_rendered), raises the per-view high-water mark and launches again when the lists overflowed.  -> (cap, geom, binning, img)"""
    static = _policy["mode"] == "static"
    cap = _policy["static"] if static else k * max(_hwm.get(dev.index, 0), 4 * P + 1024)
    while True:
        geom, binning, img = launch(cap)
        _record_forward(dev, binning, cap)
        if static:
            break
        cnt = binning[:32].view(torch.int32)[:2].cpu().tolist()
        D = cnt[0] & 0xFFFFFFFF
        _hwm[dev.index] = max(_hwm.get(dev.index, 0), int(D * 1.25 / k) + 1024)      # the mark is per view
        if not cnt[1]:
            break
        cap = k * _hwm[dev.index]
    return cap, geom, binning, img


# ------------------------------------------------------------------------------------------------------------
# screen-space gradient accumulator of the backward
# ------------------------------------------------------------------------------------------------------------
_acc_policy = {"persistent": False}
_acc_cache = {}      # (device index, P) -> zeroed (P, ACC_STRIDE) buffer kept between backwards


def set_accumulator_policy(mode):
    """"fresh" (default): every backward allocates its accumulator and clears it (a 64 B x P fill kernel).
    "persistent": ONE accumulator per (device, P) is kept between backwards; the per-Gaussian backward kernel leaves it all
    zero again (d3ga_raster_params.acc_self_clearing), so no clear is ever launched.  Valid when all rasterizer backwards
    of the process on that device are ordered on one stream (a training loop, or captured steps replayed on it) -- two
    backwards in flight on different streams would share the buffer."""
    if mode not in ("fresh", "persistent"):
        raise ValueError(mode)
    _acc_policy["persistent"] = mode == "persistent"
    if mode == "fresh":
        _acc_cache.clear()


# ------------------------------------------------------------------------------------------------------------
# tile lists from the alpha >= 1/255 box
# ------------------------------------------------------------------------------------------------------------
_tile_cull = {"override": None}


def set_tile_cull(mode):
    """None (default): every render follows its settings' `tile_cull` (off for the drop-in classes, on for renderer.render /
    render_l1 / render_pair).  True / False: process-wide override of that field for every render issued from now on -- a way
    back to the reference's lists, and an A/B switch within one build.  A captured step keeps the rule it was captured with."""
    if mode not in (None, True, False):
        raise ValueError(mode)
    _tile_cull["override"] = mode


def _tile_cull_of(requested):
    o = _tile_cull["override"]
    return bool(requested) if o is None else o


# D3GA_L1_VALUE=separate: the L1 value from its own pass over the finished image (rounds 1-3; kept for A/B runs)
_l1_policy = {"fused_value": os.environ.get("D3GA_L1_VALUE", "fused") != "separate"}


def l1_mean_forward(image, target, cell, out, dev):
    """mean |image - target| into `out` (device scalar): one partial sum per workgroup, then one workgroup adds them (index
    order: reproducible)."""
    L = _lib.lib()
    ws = torch.empty(_lib.LOSS_PARTIALS, dtype=torch.float32, device=dev)
    if cell is None:
        check(L.d3ga_l1_mean_fwd_ws(image.numel(), dptr(image), dptr(target), dptr(out), dptr(ws), stream_handle()), "d3ga_l1_mean_fwd_ws")
    else:
        check(L.d3ga_l1_mean_fwd_ws_cell(image.numel(), dptr(image), dptr(cell), dptr(out), dptr(ws), stream_handle()),
              "d3ga_l1_mean_fwd_ws_cell")


def _accumulator(P, dev):
    """-> (buffer, self_clearing)"""
    if not _acc_policy["persistent"] or P == 0:
        return torch.empty((P, _lib.ACC_STRIDE), dtype=torch.float32, device=dev), False
    key = (dev.index, P)
    buf = _acc_cache.get(key)
    if buf is None:
        if len(_acc_cache) > 8:
            _acc_cache.clear()
        buf = _acc_cache[key] = torch.zeros((P, _lib.ACC_STRIDE), dtype=torch.float32, device=dev)
    return buf, True


def last_counters(device=None):
    """dict(D, overflow, max_tile, visible) of the most recent forward on `device` (synchronises)."""
    dev = torch.cuda.current_device() if device is None else torch.device(device).index
    c = _last[dev][0][:32].view(torch.int32)[:4].cpu().tolist()
    return {"D": c[0] & 0xFFFFFFFF, "overflow": bool(c[1]), "max_tile": c[2] & 0xFFFFFFFF, "visible": c[3]}


class StageTimer:
    """Optional per-stage HIP-event timing of the rasterizer (bench.py).  While enabled the forward/backward are
    issued stage by stage through the C ABI (same kernels, same stream) with an event pair around each stage.

    `burst` (round 5): stage name -> R.  Such a stage is launched R times back to back between ITS two events and the
    elapsed time divided by R.  A single eager launch between two events on an idle queue also measures the dispatch
    latency of the kernel packet (BENCH_r04: compositing backward 121 us by the event pair against 107 us in the rocprofv3
    kernel trace of the same command); with the queue kept full the quotient is the kernel's own duration, which is what
    `roofline.achieved` is defined on.  Only for stages that may run twice on the same inputs (the compositing kernels:
    the forward rewrites the same outputs, the backward adds into an accumulator whose gradients nobody reads in this
    measuring pass)."""

    def __init__(self):
        self.enabled = False
        self.records = []          # (stage, start_event, end_event, launches between them)
        self.burst = {}

    def reset(self):
        self.records = []

    def stage(self, name, fn):
        if not self.enabled:
            return fn()
        reps = int(self.burst.get(name, 1))
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()                  # on torch's current stream == the stream the kernels are launched on
        r = fn()
        for _ in range(reps - 1):
            fn()
        b.record()
        self.records.append((name, a, b, reps))
        return r

    def summary(self):
        """stage -> (launches, mean ms per launch); call after torch.cuda.synchronize().  An event pair also sees any gap in
        which the GPU waited for the host between the two records (a Python GC pause inside one eager launch shows up as a
        multi-millisecond "kernel"), so samples longer than 5x the stage's median are left out of the mean."""
        per = {}
        for name, a, b, reps in self.records:
            per.setdefault(name, []).append((a.elapsed_time(b) / reps, reps))
        out = {}
        for name, ts in per.items():
            med = sorted(t for t, _ in ts)[len(ts) // 2]
            kept = [(t, r) for t, r in ts if t <= 5.0 * med] or ts
            out[name] = (sum(r for _, r in kept), sum(t for t, _ in kept) / len(kept))
        return out


stage_timer = StageTimer()


_scratch_sizes = {}
_prm_cache = {}          # parameter blocks by value (never mutated: _prm_variant copies one when a field has to differ)


def _scratch(P, W, H, k, cap, device, forward_only, windowed, binning=True):
    """(geom, binning, img) byte tensors for k views (k = 1: the single-view operator).  forward_only: the img buffer without
    the per-block lists of the backward (128 B per duplicate of capacity -- several hundred MB per render at a few million
    duplicates); binning=False: None for the binning buffer (a geometry-cache hit shares the first pass's).  windowed: W x H
    windows of windowed camera slots (include/d3ga.h: D3GA_CAMERA_SLOT_WINDOWED -- the window's tile grid and table)."""
    key = (P, W, H, k, cap, bool(forward_only), bool(windowed))
    sz = _scratch_sizes.get(key)
    if sz is None:                                   # (a ctypes call per render otherwise: the sizes of a training loop never change)
        sizes = (ctypes.c_int64 * 3)()
        name = "d3ga_raster_scratch_bytes_window" if windowed else "d3ga_raster_scratch_bytes_views"
        check(getattr(_lib.lib(), name)(P, W, H, k, cap, int(bool(forward_only)), sizes), name)
        if len(_scratch_sizes) > 64:
            _scratch_sizes.clear()
        sz = _scratch_sizes[key] = tuple(int(n) for n in sizes)
    new = lambda n: torch.empty(n, dtype=torch.uint8, device=device)
    return [new(sz[0]), new(sz[1]) if binning else None, new(sz[2])]


def _params(P, M, sh_degree, W, H, tanfovx, tanfovy, scale_modifier, antialiasing, prefiltered, debug, opacity_activation,
            forward_only, n_views=0, per_view_geometry=False, per_view_appearance=False, per_view_background=False, tile_cull=False):
    """The parameter block with these field values, built once per distinct value: the block of a training loop repeats, and
    building the ctypes structure costs ~6 us of an ~80 us host-bound render.  Shared (a retained graph, this cache): never
    written to -- `_prm_variant` gives the block that differs in a field."""
    key = (P, M, sh_degree, W, H, tanfovx, tanfovy, scale_modifier, antialiasing, prefiltered, debug, opacity_activation,
           forward_only, n_views, per_view_geometry, per_view_appearance, per_view_background, tile_cull)
    prm = _prm_cache.get(key)
    if prm is None:
        if len(_prm_cache) > 64:
            _prm_cache.clear()
        prm = _prm_cache[key] = RasterParams(
            P=P, M=M, sh_degree=sh_degree, W=W, H=H, tanfovx=tanfovx, tanfovy=tanfovy, scale_modifier=scale_modifier,
            antialiasing=int(antialiasing), prefiltered=int(prefiltered), debug=int(debug),
            opacity_activation=_ACTIVATIONS[opacity_activation], forward_only=int(forward_only), n_views=n_views,
            per_view_geometry=int(per_view_geometry), per_view_appearance=int(per_view_appearance),
            per_view_background=int(per_view_background), tile_cull=int(tile_cull))
        prm.cache_key = key          # (a Python attribute on the ctypes instance, not a field of the C structure: _prm_variant's key)
    return prm


def _prm_variant(prm, **fields):
    """`prm` with `fields` set to other values -- a block of its own, cached like the one it was copied from (under that
    one's key extended by the fields, so a variant of a variant nests)."""
    key = (prm.cache_key, tuple(fields.items()))
    p2 = _prm_cache.get(key)
    if p2 is None:
        if len(_prm_cache) > 64:
            _prm_cache.clear()
        p2 = _prm_cache[key] = RasterParams(**{f: getattr(prm, f) for f, _ in RasterParams._fields_})
        for f, value in fields.items():
            setattr(p2, f, value)
        p2.cache_key = key
    return p2


def _f32(t, device):
    if t is None:
        return None
    if t.dtype != torch.float32 or t.device != device:
        t = t.to(device=device, dtype=torch.float32)
    return t if t.is_contiguous() else t.contiguous()


# ------------------------------------------------------------------------------------------------------------
# the launches of one render of k views (k = 1: the single-view operator); shared with raster_views
# ------------------------------------------------------------------------------------------------------------
# gauss: (means3D, sh, colors_precomp, opacities, scales, rotations, cov3D_precomp); cam: (view matrices, full projections,
# camera rows) -- the tensors of a GaussianRasterizationSettings or the (k, .) blocks of a raster_views.CameraBatch.
def _views_of(prm):
    return max(prm.n_views, 1)


def _composite_forward(prm, cap, windowed, bg, geom, binning, img, color, invdepth, pair, l1):
    """The compositing stage: `pair` = (colors2, bg2, color2) blends a second image with the same alphas, `l1` = (target,
    target cell, loss) forms mean |color - target| while the colours are in registers, else the plain kernel."""
    L, st, pp = _lib.lib(), stream_handle(), ctypes.byref(prm)
    if pair is not None:
        colors2, bg2, color2 = pair
        stage_timer.stage("composite_fwd", lambda: check(L.d3ga_raster_composite_fwd2(
            pp, dptr(bg), dptr(bg2), dptr(geom), dptr(colors2), dptr(binning), cap, dptr(img), dptr(color), dptr(color2),
            dptr(invdepth), st), "d3ga_raster_composite_fwd2"))
    elif l1 is not None:
        target, cell, loss = l1
        # one partial sum per quadrant of every tile, then one small sum
        ws = torch.empty(4 * _views_of(prm) * ((prm.W + 15) // 16 + windowed) * ((prm.H + 15) // 16 + windowed),
                         dtype=torch.float32, device=color.device)
        stage_timer.stage("composite_fwd", lambda: check(L.d3ga_raster_composite_fwd_l1(
            pp, dptr(bg), dptr(geom), dptr(binning), cap, dptr(img), dptr(color), dptr(invdepth),
            dptr(None if cell is not None else target), dptr(cell), dptr(loss), dptr(ws), st), "d3ga_raster_composite_fwd_l1"))
    else:
        stage_timer.stage("composite_fwd", lambda: check(L.d3ga_raster_composite_fwd(
            pp, dptr(bg), dptr(geom), dptr(binning), cap, dptr(img), dptr(color), dptr(invdepth), st), "d3ga_raster_composite_fwd"))


def _launch_forward(prm, cap, windowed, gauss, cam, bg, color, radii, invdepth, pair=None, l1=None):
    """preprocess -> bin + sort -> composite into fresh scratch with room for `cap` duplicates.  -> (geom, binning, img)"""
    means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp = gauss
    view, proj, campos = cam
    k = _views_of(prm)
    geom, binning, img = _scratch(prm.P, prm.W, prm.H, k, cap, color.device, prm.forward_only, windowed)
    L = _lib.lib()
    if stage_timer.enabled or k > 1 or pair is not None or l1 is not None:
        st, pp = stream_handle(), ctypes.byref(prm)
        stage_timer.stage("preprocess", lambda: check(L.d3ga_raster_preprocess(
            pp, dptr(means3D), dptr(sh), dptr(colors_precomp), dptr(opacities), dptr(scales), dptr(rotations),
            dptr(cov3Ds_precomp), dptr(view), dptr(proj), dptr(campos), dptr(geom), dptr(binning), cap,
            dptr(radii), st), "d3ga_raster_preprocess"))
        stage_timer.stage("bin_sort", lambda: check(L.d3ga_raster_bin_sort(
            pp, dptr(geom), dptr(binning), cap, st), "d3ga_raster_bin_sort"))
        _composite_forward(prm, cap, windowed, bg, geom, binning, img, color, invdepth, pair, l1)
    else:
        # one ctypes call instead of three: the eager step is host-bound
        check(L.d3ga_raster_forward(ctypes.byref(prm), dptr(means3D), dptr(sh), dptr(colors_precomp),
                                    dptr(opacities), dptr(scales), dptr(rotations), dptr(cov3Ds_precomp),
                                    dptr(view), dptr(proj), dptr(campos), dptr(bg), dptr(geom), dptr(binning),
                                    dptr(img), cap, dptr(color), dptr(radii), dptr(invdepth), stream_handle()),
              "d3ga_raster_forward")
    return geom, binning, img


def _grad_buffers(prm, has_sh, from_sr, dev, exchanged, geo, opac, col, lead, geometry=True):
    """The gradients the per-Gaussian backward writes.  Plain: dL/dmeans3D, dL/dcov3D | dL/dscales, dL/drots of shape
    (*geo, .), dL/dopacity `opac`, dL/dcolour `col` (None: no such buffer).  `exchanged` (view-sharded training, dist.py:
    ViewShardedGrads): every gradient that leaves the op is summed over the ranks at this cut -- ONE planar buffer `flat` for
    the all-reduce and, on the SH path, the (P + 1, 3) factor of every view's rank-1 SH gradient (row P: the view's camera
    position) for ONE all-gather of (*lead, P + 1, 3) per rank.
    geometry=False (render fusion, never exchanged): no dL/dmeans3D and dL/dcov3D buffers -- the kernel keeps them in registers.
    -> (g_means3D, g_opac, g_sh, g_col, g_cov, g_scales, g_rots, cut, prm); cut: None, or what `_exchange_gradients` moves --
    (flat, factor, rasterizer input name -> its gradient, a view of `flat`)."""
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    P, cut = prm.P, None
    if not exchanged:
        g_means3D, g_opac = new(*geo, 3) if geometry else None, new(*opac)
        g_sh = new(P, prm.M, 3) if has_sh else None
        g_col = None if col is None else new(*col)
        g_cov = None if (from_sr or not geometry) else new(*geo, 6)
        g_scales = new(*geo, 3) if from_sr else None
        g_rots = new(*geo, 4) if from_sr else None
    else:
        widths = [3, 1] + ([3, 4] if from_sr else [6]) + ([] if has_sh else [3])
        flat = new(P * sum(widths))
        parts, off = [], 0
        for w in widths:
            parts.append(flat[off:off + P * w].view(P, w))
            off += P * w
        g_means3D, g_opac = parts[0], parts[1]
        g_scales, g_rots = (parts[2], parts[3]) if from_sr else (None, None)
        g_cov = None if from_sr else parts[2]
        g_sh = factor = None
        by_name = {"means3D": g_means3D, "opacities": g_opac}
        by_name.update({"scales": g_scales, "rotations": g_rots} if from_sr else {"cov3D_precomp": g_cov})
        if not has_sh:
            g_col = by_name["colors_precomp"] = parts[-1]
        else:
            # the kernel writes a view's dL/dcolour into the first P rows of its factor: the factor's own address
            g_col = factor = new(*lead, P + 1, 3)
            if _views_of(prm) > 1:                 # rows between the views' factors (include/d3ga.h: meaningful for n_views > 1)
                prm = _prm_variant(prm, factor_rows=P + 1)
        cut = (flat, factor, by_name)
    return g_means3D, g_opac, g_sh, g_col, g_cov, g_scales, g_rots, cut, prm


def _launch_backward(prm, cap, gauss, cam, bg, geom, binning, img, grad_color, grads, pair=None, g_invd=None, l1=None, deform=None):
    """composite_bwd -> preprocess_bwd.  gauss: (means3D, sh, scales, rotations, cov3D_precomp); grads: (g_means3D, g_means2D,
    g_opac, g_sh, g_col, g_cov, g_scales, g_rots); pair = (colors2, bg2, grad_color2); g_invd: the gradient of the inverse-depth
    image; l1 = (image, target, target cell, g_loss): the gradient of the fused L1 loss, formed per pixel inside the kernel.  deform = the
    (struct d3ga_cage_deform_in, _grads, _route | None) of the deform node that made means3D and the covariance (single view): the
    per-Gaussian kernel runs that node's backward as its tail (the *_deform entries); g_means3D and g_cov may then be None."""
    means3D, sh, scales, rotations, cov3Ds_precomp = gauss
    view, proj, campos = cam
    g_means3D, g_means2D, g_opac, g_sh, g_col, g_cov, g_scales, g_rots = grads
    k = _views_of(prm)
    # (k P, 16) screen-space accumulator: under set_accumulator_policy("persistent") ONE zeroed buffer per size is kept and the
    # per-Gaussian backward leaves it all zero again -- no 64 B x k P fill per backward
    acc, self_clearing = _accumulator(k * prm.P, means3D.device)
    if self_clearing != bool(prm.acc_self_clearing):
        prm = _prm_variant(prm, acc_self_clearing=int(self_clearing))
    L = _lib.lib()
    tail = () if deform is None else tuple(None if x is None else ctypes.byref(x) for x in deform)
    sfx = "" if deform is None else "_deform"
    if stage_timer.enabled or k > 1 or pair is not None or g_invd is not None:
        st, pp = stream_handle(), ctypes.byref(prm)
        if not self_clearing:
            acc.zero_()
        if pair is not None:
            colors2, bg2, grad_color2 = pair
            stage_timer.stage("composite_bwd", lambda: check(L.d3ga_raster_composite_bwd2(
                pp, dptr(bg), dptr(bg2), dptr(geom), dptr(colors2), dptr(binning), cap, dptr(img), dptr(grad_color),
                dptr(grad_color2), dptr(acc), st), "d3ga_raster_composite_bwd2"))
        elif g_invd is not None:
            stage_timer.stage("composite_bwd", lambda: check(L.d3ga_raster_composite_bwd_depth(
                pp, dptr(bg), dptr(geom), dptr(binning), cap, dptr(img), dptr(grad_color), dptr(g_invd), dptr(acc), st),
                "d3ga_raster_composite_bwd_depth"))
        elif l1 is not None:
            image, target, cell, g_loss = l1
            stage_timer.stage("composite_bwd", lambda: check(L.d3ga_raster_composite_bwd_l1(
                pp, dptr(bg), dptr(geom), dptr(binning), cap, dptr(img), dptr(image), dptr(target), dptr(cell),
                dptr(g_loss), dptr(grad_color), dptr(acc), st), "d3ga_raster_composite_bwd_l1"))
        else:
            stage_timer.stage("composite_bwd", lambda: check(L.d3ga_raster_composite_bwd(
                pp, dptr(bg), dptr(geom), dptr(binning), cap, dptr(img), dptr(grad_color), dptr(acc), st),
                "d3ga_raster_composite_bwd"))
        stage_timer.stage("preprocess_bwd", lambda: check(getattr(L, "d3ga_raster_preprocess_bwd" + sfx)(
            pp, dptr(means3D), dptr(sh), dptr(scales), dptr(rotations), dptr(cov3Ds_precomp), dptr(view), dptr(proj),
            dptr(campos), dptr(geom), dptr(acc), dptr(g_means3D), dptr(g_means2D), dptr(g_opac), dptr(g_sh),
            dptr(g_col), dptr(g_cov), dptr(g_scales), dptr(g_rots), *tail, st), "d3ga_raster_preprocess_bwd" + sfx))
    elif l1 is not None:
        image, target, cell, g_loss = l1
        check(getattr(L, "d3ga_raster_backward_l1" + sfx)(
            ctypes.byref(prm), dptr(means3D), dptr(sh), dptr(scales), dptr(rotations), dptr(cov3Ds_precomp),
            dptr(view), dptr(proj), dptr(campos), dptr(bg), dptr(geom), dptr(binning), cap, dptr(img),
            dptr(image), dptr(target), dptr(cell), dptr(g_loss), dptr(grad_color), dptr(acc), dptr(g_means3D),
            dptr(g_means2D), dptr(g_opac), dptr(g_sh), dptr(g_col), dptr(g_cov), dptr(g_scales), dptr(g_rots), *tail,
            stream_handle()), "d3ga_raster_backward_l1" + sfx)
    else:
        check(getattr(L, "d3ga_raster_backward" + sfx)(
            ctypes.byref(prm), dptr(means3D), dptr(sh), dptr(scales), dptr(rotations), dptr(cov3Ds_precomp),
            dptr(view), dptr(proj), dptr(campos), dptr(bg), dptr(geom), dptr(binning), cap, dptr(img),
            dptr(grad_color), dptr(acc), dptr(g_means3D), dptr(g_means2D), dptr(g_opac), dptr(g_sh), dptr(g_col),
            dptr(g_cov), dptr(g_scales), dptr(g_rots), *tail, stream_handle()), "d3ga_raster_backward" + sfx)


def _sh_grad_from_factors(gathered, P, M, sh_degree, means3D, scale):
    """dL/dsh (P, M, 3) = scale * sum over the views of Y(dir_v) (x) g_v, from the gathered (.., P + 1, 3) factors of all views of
    all ranks -- (world, P + 1, 3), or (world, k, P + 1, 3) from view-batched renders; row P is the view's camera position."""
    g_sh = torch.empty((P, M, 3), dtype=torch.float32, device=means3D.device)
    g = gathered.view(-1, P + 1, 3)
    check(_lib.lib().d3ga_sh_grad_from_views(P, M, sh_degree, g.shape[0], dptr(means3D), dptr(g), 3 * (P + 1), dptr(g[0, P]),
                                             3 * (P + 1), scale, dptr(g_sh), stream_handle()), "d3ga_sh_grad_from_views")
    return g_sh


def _exchange_gradients(sync, prm, cut, campos, means3D):
    """The tail of a backward whose gradients are exchanged (cut: from `_grad_buffers`): the views' camera positions into row P
    of their factors, then the collectives.  -> (parked, g_sh): parked -- the
    two-graph step (graph.CapturedCutStep) runs the collectives between the graphs, on these buffers, and the gradients come
    back REDUCED through it (returning them from the backward as well would leave the unreduced copy on the detached leaves,
    where the step adds the other loss terms' gradients); else `flat` is summed (averaged) in place and g_sh rebuilt from the
    gathered factors (None without SH)."""
    P = prm.P
    flat, factor, by_name = cut
    if factor is not None:
        factor.view(-1, P + 1, 3)[:, P].copy_(campos.reshape(_views_of(prm), -1)[:, :3])
    if getattr(sync, "deferred", False):
        sync.park(flat, factor, by_name,
                  None if factor is None else {"P": P, "M": prm.M, "sh_degree": prm.sh_degree, "means3D": means3D})
        return True, None
    gathered = sync.exchange(flat, factor)
    return False, None if factor is None else _sh_grad_from_factors(gathered, P, prm.M, prm.sh_degree, means3D, sync.scale)


# ------------------------------------------------------------------------------------------------------------
# geometry reuse between consecutive renders of the same Gaussians from the same camera
# ------------------------------------------------------------------------------------------------------------
# The reference's training step renders the same package twice (RGB, then a silhouette pass with a constant colour,
# models/trainer.py:102-110).  Projection, tile histogram, scatter and the per-tile sort depend only on
# (means3D, covariance, opacities, camera, image size), so the second call copies the first call's geometry records,
# re-evaluates only the colour (d3ga_raster_recolor) and shares its binning buffer.  A call hits the cache when its
# inputs ARE the previous call's tensors (same storage address and version counter; the cache keeps them alive, so an
# address cannot be recycled for different data).  Never used while a stream capture is in progress.
#
# OPT-IN (off by default).  A hit is decided from (data_ptr, _version, shape) only, so a write that does not bump the
# version counter is invisible to it: `p.data.add_()` / `.data.copy_()` style updates, or a kernel (this library's own C
# ABI included) writing into a preallocated buffer.  With such inputs every later render would silently reuse stale
# projection and binning.  Enable it only around the two renders of one step (`with geometry_reuse():`) -- the cache is
# dropped on exit -- or use `renderer.render_pair`, which needs no cache at all.
_reuse = {"enabled": False}
_geom_cache = {}     # device index -> dict(key, geom, binning, cap, radii, pins)


def set_geometry_reuse(enabled):
    _reuse["enabled"] = bool(enabled)
    if not enabled:
        _geom_cache.clear()


def clear_geometry_cache():
    _geom_cache.clear()


class geometry_reuse:
    """`with geometry_reuse(): rgb = render(...); sil = render(...)` -- the second render of the same package reuses the
    first one's projection / binning / sort; nothing is pinned or trusted beyond the block."""

    def __enter__(self):
        self._was = _reuse["enabled"]
        _reuse["enabled"] = True
        return self

    def __exit__(self, *exc):
        _reuse["enabled"] = self._was
        _geom_cache.clear()
        return False


def _tkey(t):
    return None if t is None else (t.data_ptr(), t._version, tuple(t.shape))


def _geometry_key(prm, cap_mode, tensors):
    return (prm.P, prm.W, prm.H, prm.tanfovx, prm.tanfovy, prm.scale_modifier, prm.prefiltered, prm.opacity_activation, prm.antialiasing, prm.tile_cull, cap_mode) + tuple(
        _tkey(t) for t in tensors)


def _empty_to_none(t):
    return None if (t is None or t.numel() == 0) else t


def _check_exactly_one(shs, colors_precomp, scales, rotations, cov3D_precomp):
    """upstream's two argument checks, with its texts"""
    if (shs is None) == (colors_precomp is None):
        raise Exception("Please provide excatly one of either SHs or precomputed colors!")
    if ((scales is None or rotations is None) and cov3D_precomp is None) or (
            (scales is not None or rotations is not None) and cov3D_precomp is not None):
        raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")


def _admit_grad_sync(grad_sync, P):
    """-> `grad_sync` when the backward exchanges its gradients through it (more than one rank, or forced: `always`; and something
    to exchange), else None."""
    if grad_sync is None or P == 0 or not (grad_sync.world > 1 or getattr(grad_sync, "always", False)):
        return None
    return grad_sync


def _verify_sync_inputs(sync, means3D, opacities, colors_precomp, sh, cov3Ds_precomp, scales, rotations):
    """the cut exchange is only valid for view-independent inputs (dist.ViewShardedGrads): checked on the first call(s)"""
    if sync is not None and hasattr(sync, "verify_inputs"):
        sync.verify_inputs({"means3D": means3D, "opacities": opacities, "colors_precomp": colors_precomp,
                            "shs": sh, "cov3D_precomp": cov3Ds_precomp, "scales": scales, "rotations": rotations})


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings, grad_sync=None, colors2=None, bg2=None, opacity_activation=None, l1_target=None,
                want_invdepth=True, deform_node=None):
        s = raster_settings
        require_cuda(means3D)
        dev = means3D.device
        if means3D.shape[0] > 0:      # upstream passes absent arguments as empty tensors
            sh, colors_precomp, scales, rotations, cov3Ds_precomp = map(
                _empty_to_none, (sh, colors_precomp, scales, rotations, cov3Ds_precomp))
        means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp = (
            _f32(t, dev) for t in (means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp))
        view, proj, campos, bg = (_f32(t, dev) for t in (s.viewmatrix, s.projmatrix, s.campos, s.bg))
        P = means3D.shape[0]
        dual = colors2 is not None and P > 0             # second image from the same pass (rasterize_gaussians_pair)
        empty_pair = colors2 is not None and P == 0      # nothing to blend: the second image is its background
        if colors2 is not None:
            colors2, bg2 = _f32(colors2.detach(), dev), _f32(bg2, dev)
        H, W = int(s.image_height), int(s.image_width)
        M = sh.shape[1] if sh is not None else 0
        tfx, tfy = float(s.tanfovx), float(s.tanfovy)
        # windowed camera slot (include/d3ga.h: D3GA_CAMERA_SLOT_WINDOWED): W x H is the crop window, campos carries (w, h, ox, oy)
        windowed = tfx == _lib.CAMERA_SLOT_WINDOWED and tfy == _lib.CAMERA_SLOT_WINDOWED and campos.numel() >= 9
        if not (tfx > 0.0 and tfy > 0.0) and not windowed:
            # tanfovx <= 0 is the in-band marker of a camera slot (cameras.CameraSlot): the kernels then read both tangents
            # from campos[3], campos[4].  Anything else non-positive (or NaN) would make them read past a 3-float campos.
            if not (tfx == 0.0 and tfy == 0.0 and campos.numel() >= 5):
                raise ValueError(f"GaussianRasterizationSettings: tanfovx / tanfovy must be positive (got {tfx}, {tfy}); only a "
                                 "camera slot (tanfovx = tanfovy = 0 with a 5-float campos: cameras.CameraSlot) reads them from the device")
        # no input requires a gradient (inference, torch.no_grad): the forward skips the per-block lists of the backward
        fwd_only = not any(ctx.needs_input_grad[:8])
        prm = _params(P, M, int(s.sh_degree), W, H, tfx, tfy, float(s.scale_modifier), bool(s.antialiasing), bool(s.prefiltered),
                      bool(s.debug), opacity_activation, fwd_only, tile_cull=_tile_cull_of(getattr(s, "tile_cull", False)))
        color = torch.empty((3, H, W), dtype=torch.float32, device=dev)
        # fused L1 image loss (rasterize_gaussians_l1): the loss VALUE is formed by the compositing forward while the colours
        # are in registers (d3ga_raster_composite_fwd_l1: one partial per quadrant, then one small sum), its gradient inside
        # the compositing backward (d3ga_raster_backward_l1): no pass over the image, no (3,H,W) gradient image
        l1_t = l1_cell = loss = None
        if l1_target is not None:
            from .graph import TensorSlot
            l1_t = l1_target.current if isinstance(l1_target, TensorSlot) else _f32(l1_target, dev)
            l1_cell = l1_target.cell if isinstance(l1_target, TensorSlot) else None
            if tuple(l1_t.shape) != (3, H, W):
                raise ValueError(f"rasterize_gaussians_l1: the target must be (3, {H}, {W}), got {tuple(l1_t.shape)}")
            loss = torch.empty((), dtype=torch.float32, device=dev)
        # the loss value from the compositing forward; else (P == 0: the image is its background, or D3GA_L1_VALUE=separate) from
        # its own pass over the finished image
        l1 = (l1_t, l1_cell, loss) if (l1_target is not None and P > 0 and colors2 is None and _l1_policy["fused_value"]) else None
        # the inverse-depth image of branch dr_aa: on request only (renderer.render* use the colour alone, renderer.py:141)
        invdepth = torch.empty((1, H, W), dtype=torch.float32, device=dev) if want_invdepth else None
        radii = torch.empty((P,), dtype=torch.int32, device=dev)
        gauss = (means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp)
        cam = (view, proj, campos)
        geo_inputs = (means3D, opacities, scales, rotations, cov3Ds_precomp, view, proj)
        color2 = torch.empty((3, H, W), dtype=torch.float32, device=dev) if dual else None
        pair = (colors2, bg2, color2) if dual else None
        use_cache = _reuse["enabled"] and P > 0 and not dual and not windowed and not torch.cuda.is_current_stream_capturing()
        key = hit = None
        if use_cache:
            key = _geometry_key(prm, ("static", _policy["static"]) if _policy["mode"] == "static" else "auto", geo_inputs)
            hit = _geom_cache.get(dev.index)
        if hit is not None and hit["key"] == key:
            cap, binning, radii = hit["cap"], hit["binning"], hit["radii"]
            geom, _unused, img = _scratch(P, W, H, 1, cap, dev, fwd_only, False, binning=False)     # img carries the per-block lists: sized by cap
            L, st, pp = _lib.lib(), stream_handle(), ctypes.byref(prm)
            stage_timer.stage("recolor", lambda: check(L.d3ga_raster_recolor(
                pp, dptr(means3D), dptr(sh), dptr(colors_precomp), dptr(campos), dptr(hit["geom"]), dptr(geom), st),
                "d3ga_raster_recolor"))
            _composite_forward(prm, cap, windowed, bg, geom, binning, img, color, invdepth, None, l1)
            _record_forward(dev, binning, cap)
        else:
            cap, geom, binning, img = _forward_with_capacity(P, 1, dev, lambda cap: _launch_forward(
                prm, cap, windowed, gauss, cam, bg, color, radii, invdepth, pair, l1))
            if use_cache:
                _geom_cache[dev.index] = {"key": key, "geom": geom, "binning": binning, "cap": cap, "radii": radii,
                                          # detached aliases: they pin the storage without keeping an autograd graph alive
                                          "pins": tuple(None if t is None else t.detach() for t in geo_inputs)}
        ctx.prm = prm
        ctx.cap = cap
        ctx.has_means2D = means2D is not None
        ctx.grad_sync = _admit_grad_sync(grad_sync, P)
        _verify_sync_inputs(ctx.grad_sync, means3D, opacities, colors_precomp, sh, cov3Ds_precomp, scales, rotations)
        ctx.dual = dual
        ctx.l1 = l1_target is not None and P > 0 and not dual
        # render fusion (cage_deform.claim_for_render): the deform node that made means3D and the covariance runs the per-Gaussian
        # part of its backward as the tail of this operator's.  Single view on the full raster, gradients not exchanged.
        if deform_node is not None and (windowed or ctx.grad_sync is not None or P == 0 or cov3Ds_precomp is None or fwd_only):
            from .cage_deform import release_claim
            release_claim(*deform_node)
            deform_node = None
        ctx.deform_node = deform_node                    # (node, the claim's token) | None
        if l1_target is not None and l1 is None:
            l1_mean_forward(color, l1_t, l1_cell, loss, dev)
        _last_img[dev.index] = (img, W, H, geom, P)
        ctx.save_for_backward(means3D, sh, scales, rotations, cov3Ds_precomp, view, proj, campos, bg, geom, binning, img,
                              colors2, bg2, color if ctx.l1 else None, l1_t if ctx.l1 else None, l1_cell if ctx.l1 else None)
        # (the inverse-depth image IS differentiable, as on branch dr_aa: with set_materialize_grads(False) an unused one costs nothing)
        ctx.mark_non_differentiable(radii)
        ctx.set_materialize_grads(False)                 # no zero-filled (P,) / (H,W) gradients for radii / invdepth per step
        if l1_target is not None:
            return color, radii, invdepth, loss
        if dual:
            return color, radii, invdepth, color2
        if empty_pair:
            return color, radii, invdepth, bg2.reshape(3, 1, 1).expand(3, H, W).contiguous()
        return color, radii, invdepth

    @staticmethod
    def backward(ctx, grad_color, _grad_radii, _grad_invdepth, grad_color2=None):
        (means3D, sh, scales, rotations, cov3Ds_precomp, view, proj, campos, bg, geom, binning, img, colors2,
         bg2, image, l1_t, l1_cell) = ctx.saved_tensors
        prm, dev, P = ctx.prm, means3D.device, means3D.shape[0]
        dual = ctx.dual
        g_loss = None
        if ctx.l1:                                       # the 4th output was the fused L1 loss: its incoming gradient
            g_loss, grad_color2 = grad_color2, None
            if g_loss is not None:
                g_loss = _f32(g_loss, dev).reshape(1)
        g_invd = None
        if _grad_invdepth is not None:                   # a loss on the inverse-depth image (branch dr_aa's depth regularisation)
            if dual or ctx.l1:
                raise NotImplementedError("a gradient of the inverse-depth image is implemented for the single-image rasterizer call only "
                                          "(not for rasterize_gaussians_pair / rasterize_gaussians_l1)")
            g_invd = _f32(_grad_invdepth, dev).reshape(prm.H, prm.W)
        if grad_color is None and g_loss is None and g_invd is None:        # only the second image was used (or nothing at all)
            grad_color = torch.zeros((3, prm.H, prm.W), dtype=torch.float32, device=dev)
        grad_color = _f32(grad_color, dev)
        if dual:
            grad_color2 = (torch.zeros_like(grad_color) if grad_color2 is None else _f32(grad_color2, dev))
        has_sh, from_sr, sync = sh is not None, cov3Ds_precomp is None, ctx.grad_sync
        deform = deposit = node = None
        if ctx.deform_node is not None:
            from .cage_deform import deposit_on, fused_tail_structs, holds_claim
            # (a later render of the package may have revoked the claim; a retain_grad() or hook since the render ends it here)
            node = ctx.deform_node[0] if holds_claim(*ctx.deform_node) else None
        # a held claim: dL/dmeans3D and dL/dcov stay in the kernel's registers (no buffers), the node's share is deposited on it
        g_means3D, g_opac, g_sh, g_col, g_cov, g_scales, g_rots, cut, prm = _grad_buffers(
            prm, has_sh, from_sr, dev, exchanged=sync is not None, geo=(P,), opac=(P, 1), col=None if has_sh else (P, 3), lead=(),
            geometry=node is None)
        g_means2D = torch.empty((P, 3), dtype=torch.float32, device=dev)
        if node is not None:
            *deform, deposit = fused_tail_structs(node)
        _launch_backward(prm, ctx.cap, (means3D, sh, scales, rotations, cov3Ds_precomp), (view, proj, campos), bg, geom, binning, img,
                         grad_color, (g_means3D, g_means2D, g_opac, g_sh, g_col, g_cov, g_scales, g_rots),
                         (colors2, bg2, grad_color2) if dual else None, g_invd,
                         (image, l1_t, l1_cell, g_loss) if g_loss is not None else None, deform)
        if deposit is not None:
            deposit_on(node, deposit)
        if sync is not None:
            parked, g_sh = _exchange_gradients(sync, prm, cut, campos, means3D)
            if parked:
                return (None, g_means2D if ctx.has_means2D else None) + (None,) * 14
            if has_sh:
                g_col = None
        return (g_means3D, g_means2D if ctx.has_means2D else None, g_sh, g_col, g_opac, g_scales, g_rots, g_cov, None,
                None, None, None, None, None, None, None)


_ACTIVATIONS = {None: 0, "none": 0, "sigmoid": 1}       # D3GA_OPACITY_SIGMOID


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings, grad_sync=None, opacity_activation=None, want_invdepth=True, deform_node=None):
    """opacity_activation="sigmoid" (extension over upstream): `opacities` holds the raw logits and the sigmoid of
    models/cage_net.py:247 runs inside the per-Gaussian kernels, forward and backward.
    deform_node (all three operators; renderer.render passes it): (node, token) -- the deform node claimed for this render
    (cage_deform.claim_for_render) -- its backward's per-Gaussian part then runs as the tail of this operator's, and means3D and
    cov3Ds_precomp receive no gradient of their own."""
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                     cov3Ds_precomp, raster_settings, grad_sync, None, None, opacity_activation, None, want_invdepth,
                                     deform_node)


def rasterize_gaussians_l1(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                           raster_settings, target, grad_sync=None, opacity_activation=None, want_invdepth=True, deform_node=None):
    """The render AND its L1 image loss (utils/loss_utils.py:29: mean |image - target|) from one operator (extension):
    returns (color, radii, invdepth, loss).  The gradient of `loss` is formed per pixel inside the compositing backward,
    so no (3,H,W) gradient image is written or read (one full-image kernel and 50 MB of traffic less per frame at 1080p);
    `color` stays differentiable as usual and both gradients add.  `target`: (3,H,W) tensor or a `graph.TensorSlot`."""
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                     cov3Ds_precomp, raster_settings, grad_sync, None, None, opacity_activation, target, want_invdepth,
                                     deform_node)


def rasterize_gaussians_pair(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                             raster_settings, colors2, bg2, grad_sync=None, opacity_activation=None, want_invdepth=True,
                             deform_node=None):
    """Two images from ONE pass: the usual one and `colors2` (P,3; constants, no gradient) blended with the same alphas over
    `bg2`.  Returns (color, radii, invdepth, color2).  Gradients of both images reach the geometry and the opacities."""
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                     cov3Ds_precomp, raster_settings, grad_sync, colors2, bg2, opacity_activation, None, want_invdepth,
                                     deform_node)


class GaussianRasterizer(nn.Module):
    """`grad_sync` (optional, not in upstream): a d3ga_amd.dist.ViewShardedGrads -- the gradients returned by the
    backward are then already summed/averaged over the ranks of the group (each rank renders its own camera)."""

    def __init__(self, raster_settings, grad_sync=None, opacity_activation=None):
        super().__init__()
        self.raster_settings = raster_settings
        self.grad_sync = grad_sync
        self.opacity_activation = opacity_activation      # "sigmoid": `opacities` are logits (fused D8 activation)
        self.want_invdepth = True                         # False: [2] of the result is None (the forward skips the depth image)

    def markVisible(self, positions):
        """Boolean (P,) mask: view-space z > 0.2 (upstream _C.mark_visible)."""
        require_cuda(positions)
        with torch.no_grad():
            p = _f32(positions, positions.device)
            view = _f32(self.raster_settings.viewmatrix, positions.device)
            vis = torch.empty((p.shape[0],), dtype=torch.uint8, device=p.device)
            check(_lib.lib().d3ga_raster_mark_visible(p.shape[0], dptr(p), dptr(view), dptr(vis), stream_handle()),
                  "d3ga_raster_mark_visible")
        return vis.bool()

    def forward(self, means3D, means2D, opacities, shs: Optional[torch.Tensor] = None,
                colors_precomp: Optional[torch.Tensor] = None, scales: Optional[torch.Tensor] = None,
                rotations: Optional[torch.Tensor] = None, cov3D_precomp: Optional[torch.Tensor] = None):
        _check_exactly_one(shs, colors_precomp, scales, rotations, cov3D_precomp)
        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                   self.raster_settings, self.grad_sync, self.opacity_activation, self.want_invdepth)


def last_tile_lists(W, H, device=None):
    """tile_lists() of the most recent forward on `device`."""
    dev = torch.cuda.current_device() if device is None else torch.device(device).index
    binning, cap = _last[dev]
    return tile_lists(binning, W, H, cap)


def last_termination(device=None):
    """(final_T (H,W) float32, n_contrib (H,W) int32) of the most recent forward on `device`: the per-pixel termination the
    backward reads (views into the forward's image scratch, layout from d3ga_raster_img_layout; inspection / tests -- the
    shared-decision parity test hands them to the oracle's backward)."""
    dev = torch.cuda.current_device() if device is None else torch.device(device).index
    img, W, H = _last_img[dev][:3]
    off = (ctypes.c_int64 * 2)()
    check(_lib.lib().d3ga_raster_img_layout(W, H, off), "d3ga_raster_img_layout")
    n = 4 * W * H
    return (img[off[0]:off[0] + n].view(torch.float32).view(H, W), img[off[1]:off[1] + n].view(torch.int32).view(H, W))


def last_block_lists(device=None):
    """(blk_count (tiles,16) int64, blk_list (16 x capacity, 2) int64 {1-based tile-list position, Gaussian index}) of the most
    recent forward that was followed by (or may be followed by) a backward on `device` -- views decoded from its image scratch
    (d3ga_raster_img_layout_blocks; inspection / tests).  Block b of a tile whose list is [begin, end) starts at row
    16 begin + b (end - begin) of blk_list; blk_count is the prefix the backward walks."""
    dev = torch.cuda.current_device() if device is None else torch.device(device).index
    img, W, H = _last_img[dev][:3]
    off = (ctypes.c_int64 * 2)()
    check(_lib.lib().d3ga_raster_img_layout_blocks(W, H, off), "d3ga_raster_img_layout_blocks")
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    if img.numel() <= off[1]:
        raise RuntimeError("the last forward was a forward_only render: it has no block lists")
    cnt = img[off[0]:off[0] + 64 * tiles].view(torch.int32).view(tiles, 16).long()
    n = (img.numel() - off[1]) // 8
    lst = img[off[1]:off[1] + 8 * n].view(torch.int32).view(n, 2).long()
    return cnt, lst


def last_alpha_decisions(gid, px, py, device=None):
    """(ok (n,) bool, alpha (n,) float32): the compositing forward's own alpha and "touches the pixel" decision for the listed
    (Gaussian, pixel) pairs over the geometry records of the most recent forward (d3ga_selftest_alpha; tests)."""
    dev = torch.cuda.current_device() if device is None else torch.device(device).index
    geom, P = _last_img[dev][3:5]
    d = geom.device
    gid, px, py = (torch.as_tensor(t, dtype=torch.int32).to(d).contiguous() for t in (gid, px, py))
    n = gid.numel()
    ok = torch.zeros(max(n, 1), dtype=torch.uint8, device=d)
    alpha = torch.zeros(max(n, 1), dtype=torch.float32, device=d)
    check(_lib.lib().d3ga_selftest_alpha(P, dptr(geom), n, dptr(gid), dptr(px), dptr(py), dptr(ok), dptr(alpha), stream_handle()),
          "d3ga_selftest_alpha")
    return ok[:n].bool(), alpha[:n]


def tile_lists(binning, W, H, d_capacity):
    """(tile_start (tiles+1,) int64, point_list (D,) int64, keys (D,) int64) views decoded from a binning buffer
    (inspection / tests; layout from d3ga_raster_binning_layout)."""
    off = (ctypes.c_int64 * 6)()
    check(_lib.lib().d3ga_raster_binning_layout(W, H, d_capacity, off), "d3ga_raster_binning_layout")
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    start = binning[off[2]:off[2] + 4 * (tiles + 1)].view(torch.int32).long() & 0xFFFFFFFF
    D = min(int(start[-1]), d_capacity)
    keys = binning[off[4]:off[4] + 8 * D].view(torch.int64)
    plist = binning[off[5]:off[5] + 4 * D].view(torch.int32).long()
    return start, plist, keys
