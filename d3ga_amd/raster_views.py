"""View-batched rasterization: k cameras of ONE set of Gaussians in one grid per stage (include/d3ga.h: d3ga_raster_params::n_views).

No counterpart upstream -- the reference renders one camera per call (renderer.py:69) and averages the losses of a batch of
frames (train.py:218-221).  A single avatar view leaves two thirds of the chip idle in the binning and compositing launches
(DESIGN.md sec. 4); k views of the same pose are one tall frame for those stages.  Per view the arithmetic is that of the
single-view operator, so every image equals `rasterize_gaussians` from that camera and the gradients equal the sum over the k
single-view backwards.

    CameraBatch(k, width, height)            k cameras in one static device buffer (graph-replayable: `set(batches)`)
    rasterize_gaussians_views(...)           -> (colors (k,3,H,W), radii (k,P), loss | None)
"""
import torch

from . import _lib
from ._lib import require_cuda
from .cameras import Camera, crop_window
from . import rasterizer as _R


class CameraBatch:
    """k cameras of one raster size in ONE device buffer: view matrices (k,16) | full projections (k,16) | centres + tangents
    (k,5).  The kernels read tan(FoV/2) per view from the buffer (the camera-slot convention of include/d3ga.h: the settings
    carry tanfovx = 0), so the cameras of a batch may differ in everything but the raster size, and a captured step is replayed
    with other cameras after `set()` -- one asynchronous H2D copy.

    windowed=True: width x height is the CROP WINDOW every view pastes to (lib/batch.py:186-198, renderer.py:36-47), and the views
    may differ in raster size and principal point: the centre rows grow to (k,9) with (w, h, ox, oy) behind the tangents and the
    kernels rasterize each view's window directly (include/d3ga.h: D3GA_CAMERA_SLOT_WINDOWED)."""

    def __init__(self, n_views, width, height, device="cuda", windowed=False):
        self.n_views, self.image_width, self.image_height = int(n_views), int(width), int(height)
        self.windowed = bool(windowed)
        k = self.n_views
        c = 9 if self.windowed else 5
        self._c = c
        self.buffer = torch.zeros((32 + c) * k, dtype=torch.float32, device=torch.device(device))
        self.viewmatrices = self.buffer[:16 * k].view(k, 16)
        self.projmatrices = self.buffer[16 * k:32 * k].view(k, 16)
        self.campos = self.buffer[32 * k:].view(k, c)
        self._host = torch.zeros((32 + c) * k, dtype=torch.float32)
        if self.buffer.is_cuda:
            self._host = self._host.pin_memory()
        self._host_np = self._host.numpy()
        self._event = None

    def set(self, batches):
        """batches: k dicts with the reference's camera keys (R, T, FoVx, FoVy, width, height: lib/cameras.py:14-26)."""
        k = self.n_views
        if len(batches) != k:
            raise ValueError(f"CameraBatch holds {k} cameras, got {len(batches)}")
        if self._event is not None:
            self._event.synchronize()                 # the copy that last read the staging buffer has run
        h = self._host_np
        rows = []
        for v, b in enumerate(batches):
            if self.windowed:
                w, hh, ox, oy, W, H = crop_window(b)
                if (W, H) != (self.image_width, self.image_height):
                    raise ValueError(f"CameraBatch is a {self.image_width}x{self.image_height} window; view {v}'s crop pastes to {W}x{H}")
                rows.append((w, hh, ox, oy))
            elif int(b["width"]) != self.image_width or int(b["height"]) != self.image_height:
                raise ValueError(f"CameraBatch is {self.image_width}x{self.image_height}; view {v} is {b['width']}x{b['height']}")
        c = self._c
        for v, b in enumerate(batches):
            m = Camera.pack_host_cached(b)        # view (16) | projection (16) | full (16) | centre (3) | tan(FoVx/2), tan(FoVy/2)
            h[16 * v:16 * v + 16] = m[0:16]
            h[16 * k + 16 * v:16 * k + 16 * v + 16] = m[32:48]
            o = 32 * k + c * v
            h[o:o + 3] = m[48:51]
            h[o + 3:o + 5] = m[51:53]
            if self.windowed:
                h[o + 5:o + 9] = rows[v]
        self.buffer.copy_(self._host, non_blocking=True)
        if self.buffer.is_cuda:
            self._event = torch.cuda.Event()
            self._event.record()
        return self


class _RasterizeViews(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, cams, bg, sh_degree,
                scale_modifier, antialiasing, opacity_activation, l1_targets, colors2=None, bg2=None, grad_sync=None, tile_cull=False):
        require_cuda(means3D)
        dev = means3D.device
        f32 = lambda t: _R._f32(t, dev)
        means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, bg = map(
            f32, (means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, bg))
        _R._check_exactly_one(sh, colors_precomp, scales, rotations, cov3Ds_precomp)
        k, W, H = cams.n_views, cams.image_width, cams.image_height
        windowed = getattr(cams, "windowed", False)
        if windowed and grad_sync is not None:
            raise ValueError("rasterize_gaussians_views: grad_sync (camera-sharded exchange) is not available with windowed cameras "
                             "(CameraBatch(windowed=True)); render the windows without it")
        # a batch of FRAMES: every view brings its own geometry (k,P,.) -- the avatar deformed per pose -- and shares the appearance
        per_view = means3D.dim() == 3
        P = means3D.shape[-2]
        geo = [t for t in (means3D, scales, rotations, cov3Ds_precomp) if t is not None]
        if any((t.dim() == 3) != per_view for t in geo) or (per_view and any(t.shape[0] != k for t in geo)):
            raise ValueError("rasterize_gaussians_views: means3D and the covariance inputs must all be (P,.) or all be (k,P,.)")
        # per-view appearance (the ColorField configuration: colour and opacity evaluated per frame / camera): opacities (k,P[,1]) and
        # colors_precomp (k,P,3) -- the wrapper below has given both the same form; the gradients come back per view
        pva = _appearance_per_view(opacities, colors_precomp, sh, k, P)
        ctx.opacities_shape = tuple(opacities.shape)
        pvb = _background_per_view(bg, k)
        if pva and grad_sync is not None:
            raise ValueError("rasterize_gaussians_views: grad_sync (camera-sharded exchange at the cut) needs view-independent appearance; "
                             "per-view colours and opacities are reduced at the parameters (dist.BucketedGradReducer)")
        M = sh.shape[1] if sh is not None else 0
        fwd_only = not any(ctx.needs_input_grad[:7])
        dual = colors2 is not None
        if dual and l1_targets is not None:
            raise ValueError("rasterize_gaussians_views: the fused L1 loss and a second colour set cannot be combined")
        if dual:
            colors2, bg2 = f32(colors2.detach()), f32(bg2)
            if tuple(colors2.shape) != (P, 3) or bg2.numel() != 3:
                raise ValueError("rasterize_gaussians_views: colors2 is (P,3) and bg2 (3,), shared by the views")
        marker = _lib.CAMERA_SLOT_WINDOWED if windowed else 0.0         # camera slots: tangents (and windows) from the device rows
        prm = _R._params(P, M, int(sh_degree), W, H, marker, marker, float(scale_modifier), bool(antialiasing), False, False,
                         opacity_activation, fwd_only, k, per_view, pva, pvb, _R._tile_cull_of(tile_cull))
        colors2_img = torch.empty((k, 3, H, W), dtype=torch.float32, device=dev) if dual else None
        colors = torch.empty((k, 3, H, W), dtype=torch.float32, device=dev)
        radii = torch.empty((k, P), dtype=torch.int32, device=dev)
        loss = tgt = None
        if l1_targets is not None:
            tgt = f32(l1_targets)
            if tuple(tgt.shape) != (k, 3, H, W):
                raise ValueError(f"rasterize_gaussians_views: the targets must be ({k}, 3, {H}, {W}), got {tuple(tgt.shape)}")
            loss = torch.empty((), dtype=torch.float32, device=dev)
        gauss = (means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp)
        cam = (cams.viewmatrices, cams.projmatrices, cams.campos)
        # nothing to blend (P == 0): every image is its background, the loss and the second image are formed from that
        pair = (colors2, bg2, colors2_img) if (dual and P > 0) else None
        l1 = (tgt, None, loss) if (tgt is not None and P > 0) else None
        cap, geom, binning, img = _R._forward_with_capacity(P, k, dev, lambda cap: _R._launch_forward(
            prm, cap, windowed, gauss, cam, bg, colors, radii, None, pair, l1))
        if tgt is not None and l1 is None:
            _R.l1_mean_forward(colors, tgt, None, loss, dev)
        if dual and pair is None:
            colors2_img.copy_(bg2.view(1, 3, 1, 1).expand_as(colors2_img))
        ctx.prm, ctx.cap, ctx.cams = prm, cap, cams
        ctx.l1 = l1 is not None
        ctx.dual, ctx.per_view, ctx.pva = dual, per_view, pva
        # camera-sharded training (d3ga_amd/dist.py: ViewShardedGrads): every gradient that leaves this op is summed over the ranks
        # at this cut -- this rank's k views arrive already summed, their k SH factors travel in one all-gather
        ctx.grad_sync = _R._admit_grad_sync(grad_sync, P)
        if ctx.grad_sync is not None and per_view:
            raise ValueError("rasterize_gaussians_views: grad_sync needs view-independent geometry (k cameras of one pose); a batch of "
                             "frames is reduced at the parameters (dist.GradReducer)")
        _R._verify_sync_inputs(ctx.grad_sync, means3D, opacities, colors_precomp, sh, cov3Ds_precomp, scales, rotations)
        ctx.save_for_backward(means3D, sh, scales, rotations, cov3Ds_precomp, bg, geom, binning, img,
                              colors if ctx.l1 else None, tgt if ctx.l1 else None, colors2, bg2)
        ctx.mark_non_differentiable(radii)
        ctx.set_materialize_grads(False)
        if dual:
            return colors, radii, colors2_img
        return (colors, radii, loss) if tgt is not None else (colors, radii)

    @staticmethod
    def backward(ctx, grad_colors, _grad_radii, grad_third=None):
        means3D, sh, scales, rotations, cov3Ds_precomp, bg, geom, binning, img, image, tgt, colors2, bg2 = ctx.saved_tensors
        prm, cams, dev, P, k = ctx.prm, ctx.cams, means3D.device, ctx.prm.P, ctx.prm.n_views
        if P == 0:
            return (None,) * 18
        g_loss = grad_colors2 = None
        if ctx.l1 and grad_third is not None:
            g_loss = _R._f32(grad_third, dev).reshape(1)
        if ctx.dual:
            grad_colors2 = torch.zeros((k, 3, prm.H, prm.W), dtype=torch.float32, device=dev) if grad_third is None else _R._f32(grad_third, dev)
        if grad_colors is None and g_loss is None:
            grad_colors = torch.zeros((k, 3, prm.H, prm.W), dtype=torch.float32, device=dev)
        grad_colors = _R._f32(grad_colors, dev)
        has_sh, from_sr, sync = sh is not None, cov3Ds_precomp is None, ctx.grad_sync
        geo = (k, P) if ctx.per_view else (P,)                 # a batch of frames: geometry gradients per view
        # per-view appearance: (k,P[,1]) and (k,P,3), per view; SH: the per-view factors of the rank-1 SH gradient (scratch)
        g_means3D, g_opac, g_sh, g_col, g_cov, g_scales, g_rots, cut, prm = _R._grad_buffers(
            prm, has_sh, from_sr, dev, exchanged=sync is not None, geo=geo, opac=ctx.opacities_shape if ctx.pva else (P, 1),
            col=(k, P, 3) if (has_sh or ctx.pva) else (P, 3), lead=(k,))
        _R._launch_backward(prm, ctx.cap, (means3D, sh, scales, rotations, cov3Ds_precomp), (cams.viewmatrices, cams.projmatrices, cams.campos),
                            bg, geom, binning, img, grad_colors, (g_means3D, None, g_opac, g_sh, g_col, g_cov, g_scales, g_rots),
                            (colors2, bg2, grad_colors2) if ctx.dual else None, None,
                            (image, tgt, None, g_loss) if g_loss is not None else None)
        if sync is not None:
            parked, g_sh = _R._exchange_gradients(sync, prm, cut, cams.campos, means3D)
            if parked:
                return (None,) * 18
        return (g_means3D, g_sh, g_col if sh is None else None, g_opac, g_scales, g_rots, g_cov,
                None, None, None, None, None, None, None, None, None, None, None)


def _appearance_per_view(opacities, colors_precomp, sh, k, P):
    """True for per-view opacities (k,P) | (k,P,1) with colours (k,P,3); False for the shared (P,) | (P,1) and (P,3).  Anything else
    -- a leading dimension that is not k, SH colours with per-view opacities, one of the two per view and the other not -- raises."""
    def form(t, width, what):
        if t is None:
            return None
        shared = ((P,), (P, 1)) if width == 1 else ((P, width),)
        per_view = ((k, P), (k, P, 1)) if width == 1 else ((k, P, width),)
        shape = tuple(t.shape)
        if shape in shared:
            return False
        if shape in per_view:
            return True
        raise ValueError(f"rasterize_gaussians_views: {what} must be {' or '.join(map(str, shared))} (shared by the {k} views) or "
                         f"{' or '.join(map(str, per_view))} (one per view), got {shape}")
    op, col = form(opacities, 1, "opacities"), form(colors_precomp, 3, "colors_precomp")
    if op and sh is not None:
        raise ValueError("rasterize_gaussians_views: per-view opacities need precomputed colours (k,P,3); SH colours are view-dependent "
                         "already and their coefficients are shared")
    if col is not None and op != col:
        raise ValueError("rasterize_gaussians_views: opacities and colors_precomp must both be shared (P,.) or both per view (k,P,.)")
    return bool(op)


def _background_per_view(bg, k):
    if tuple(bg.shape) in ((3,), (1, 3)):
        return False
    if tuple(bg.shape) == (k, 3):
        return True
    raise ValueError(f"rasterize_gaussians_views: bg must be (3,) (shared by the {k} views) or ({k}, 3) (one per view), got {tuple(bg.shape)}")


def rasterize_gaussians_views(means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, cameras, bg, sh_degree=0,
                              scale_modifier=1.0, antialiasing=False, opacity_activation=None, l1_targets=None, colors2=None, bg2=None,
                              grad_sync=None, tile_cull=False):
    """k views in one grid per stage.  cameras: a CameraBatch; bg (3,) shared by the views or (k,3), one per view (the reference
    draws a background per frame, models/trainer.py:95-100).
    Geometry: means3D (P,3) with cov3Ds_precomp (P,6) | scales + rotations -- k CAMERAS of one set of Gaussians -- or all of them
    (k,P,.) -- k FRAMES, the avatar deformed per pose (the reference's batch, train.py:218-221).  Appearance: opacities (P,[1]) and
    sh | colors_precomp (P,3) shared by the views, or -- the ColorField configuration, colour and opacity evaluated per frame
    (models/cage_net.py:232-258) -- opacities (k,P[,1]) with colors_precomp (k,P,3), one per view; a shared one of the two beside a
    per-view one is broadcast to (k,P,.) here.
    -> (colors (k,3,H,W), radii (k,P)); with l1_targets (k,3,H,W): (colors, radii, loss), loss = mean |colors - targets| over all k
    images (= the mean over the frames of the reference's per-frame l1_loss: equal sizes), its gradient formed inside the compositing
    backward; with colors2 (P,3) + bg2: (colors, radii, colors2_image (k,3,H,W)) -- the reference's RGB + silhouette pair
    (models/trainer.py:102-110) from one pass, colors2 constant.  Gradients as `rasterize_gaussians`: summed over the views for
    shared inputs, per view for (k,P,.) geometry.  grad_sync: a dist.ViewShardedGrads -- the returned gradients are then already
    averaged over the ranks of a camera-sharded run (every rank renders its own k cameras of the pose); not with per-view appearance.
    tile_cull: bin by the alpha >= 1/255 box (GaussianRasterizationSettings.tile_cull; rasterizer.set_tile_cull overrides it)."""
    k = cameras.n_views
    if k > 1 and opacities is not None and colors_precomp is not None:
        P = means3D.shape[-2]
        op_pv = opacities.dim() == 3 or (opacities.dim() == 2 and tuple(opacities.shape) != (P, 1))
        if op_pv and colors_precomp.dim() == 2:
            colors_precomp = colors_precomp.unsqueeze(0).expand(k, *colors_precomp.shape)      # (autograd sums the views back)
        elif colors_precomp.dim() == 3 and not op_pv:
            opacities = opacities.reshape(1, P, 1).expand(k, P, 1)
    return _RasterizeViews.apply(means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, cameras, bg,
                                 sh_degree, scale_modifier, antialiasing, opacity_activation, l1_targets, colors2, bg2, grad_sync, tile_cull)
