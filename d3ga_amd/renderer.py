"""Drop-in for the reference's renderer.py: `render(batch, pkg, bg_color, colors_precomp=None, measure_time=False,
solid_bg=True, fast=False, detach=[]) -> {"render": (3,H',W')}` (renderer.py:69-145), on the MI355X rasterizer.
"""
import torch

from .cameras import CAMERA_SLOT_WINDOWED, batch_to_camera, crop_window, is_cropped, window_camera
from .rasterizer import GaussianRasterizationSettings, rasterize_gaussians, rasterize_gaussians_l1, rasterize_gaussians_pair

bg_colors = {"white": (1.0, 1.0, 1.0), "black": (0.0, 0.0, 0.0)}


_zeros = {}


def _zero_leaf(like):
    key = (like.device, tuple(like.shape))
    z = _zeros.get(key)
    if z is None:
        if len(_zeros) > 16:
            _zeros.clear()
        z = _zeros[key] = torch.zeros(like.shape, dtype=torch.float32, device=like.device)
    return z.detach().requires_grad_(True)


def paste(img, crop):
    """Undo the symmetric-FoV padding of lib/batch.py:186-198 (renderer.py:36-47)."""
    left_w, right_w, top_h, bottom_h, W, H = crop[0], crop[1], crop[2], crop[3], int(crop[4]), int(crop[5])
    # identity crops (centred principal point) are skipped: a no-op slice still costs a zero-fill + copy of the whole
    # image in its backward
    if W < img.shape[2]:
        img = img[:, :, :W] if left_w > right_w else img[:, :, -W:]
    if H < img.shape[1]:
        img = img[:, :H, :] if top_h > bottom_h else img[:, -H:, :]
    return img


def render_pair(batch, pkg, bg_color, colors2, bg_color2, grad_sync=None, crop_window=False):
    """The two renders of the reference's training step (models/trainer.py:102-110: `render(frame, pkg, bg)` and
    `render(frame, pkg, colors_precomp=pkg["silhouette_rgb"], bg_color=zeros)`) from ONE pass over the same geometry:
    -> {"render": (3,H',W'), "render2": (3,H',W')}.  Same images and the same summed gradients as the two calls (colors2
    is treated as constant, as the reference's silhouette colours are); use the two calls when `detach` differs.  crop_window: as for
    `render`."""
    out = render(batch, pkg, bg_color, grad_sync=grad_sync, _pair=(colors2, bg_color2), crop_window=crop_window)
    return out


def render_l1(batch, pkg, bg_color, target, grad_sync=None, crop_window=False):
    """`render(batch, pkg, bg_color)` and `l1_loss(render, target)` (utils/loss_utils.py:29, train.py:190) from one operator:
    -> {"render": (3,H',W'), "l1": scalar}.  Same image, same loss, same gradients as the two calls; the loss gradient is
    formed inside the compositing backward instead of travelling through a (3,H,W) gradient image.  `target`: a tensor of
    the render's shape or a `graph.TensorSlot`.  With an off-centre crop (lib/batch.py:186-198: the loss lives on the cropped
    window, not on the raster) the two calls are made instead -- unless crop_window=True (see `render`): the window is then rendered
    directly and the loss stays fused (one operator)."""
    windowed = crop_window or _windowed_slot(batch)
    if is_cropped(batch) and not windowed:
        from .losses import l1_loss
        img = render(batch, pkg, bg_color, grad_sync=grad_sync)["render"]
        return {"render": img, "l1": l1_loss(img, target)}
    return render(batch, pkg, bg_color, grad_sync=grad_sync, _l1=target, crop_window=crop_window)


def _windowed_slot(batch):
    slot = batch.get("camera_slot")
    return slot is not None and getattr(slot, "windowed", False)


def render_views(batches, pkg, bg_color, targets=None, cameras=None, colors2=None, bg_color2=None, grad_sync=None, tile_cull=False):
    """k views in one pass (extension; the reference renders one camera per call and averages the losses of a batch of frames,
    train.py:218-221): -> {"render": (k,3,H,W)}; with targets (k,3,H,W) also "l1" = the mean over the views of `l1_loss(render,
    target)` (its gradient formed inside the compositing backward); with colors2 (P,3) + bg_color2 (3,) also "render2" (k,3,H,W), the
    reference's silhouette pass (models/trainer.py:102-110) from the same pass.  bg_color: (3,) shared, or (k,3) one per view (the
    reference's random background per frame, models/trainer.py:95-100).
    pkg: one package seen from k CAMERAS -- or a LIST of k packages, one per FRAME of the batch (the avatar deformed per pose:
    their means3D and covariances are stacked to (k,P,.)).  Appearance: `shs` and `sh_degree` must be the same in all packages;
    `rgb` / `opacities` / `opacity_logits` that are the same tensor in every package are shared, ones that differ (the ColorField
    configuration, use_shs false: colour and opacity evaluated per frame) are stacked to (k,P,.) and rendered per view.  One package
    seen from k cameras may carry `rgb` (k,P,3) and `opacities` (k,P,1) itself (ColorField evaluated once per camera).  Every image
    equals `render(batch_v, pkg_v, bg_color_v)["render"]`, the gradients equal the sum over the k calls (d3ga_amd/raster_views.py).
    Views with off-centre crops or different raster sizes (lib/batch.py:186-198: every camera's own padded raster) are rendered
    through their crop windows (CameraBatch(windowed=True), include/d3ga.h: D3GA_CAMERA_SLOT_WINDOWED): every image is then
    `paste(render(batch_v, ...)["render"], crop_v)`, (k,3,H,W) with (W,H) = crop[4], crop[5], which must be the same for all views;
    targets are (k,3,H,W) windows.  Centred views of one raster size take the full-raster path.  cameras: a `raster_views.CameraBatch`
    to reuse (a captured step keeps one and calls `cameras.set(batches)` before every replay); batches may then be None.
    tile_cull: bin by the alpha >= 1/255 box as `render` does (GaussianRasterizationSettings.tile_cull).  Off by default here: the
    batch's tile lists are then the reference's, view by view."""
    from .raster_views import CameraBatch, rasterize_gaussians_views
    frames = pkg if isinstance(pkg, (list, tuple)) else None
    if frames is not None:
        first = frames[0]
        for f in frames[1:]:
            if f.get("shs") is not first.get("shs"):
                raise ValueError("render_views: the frames of a batch share their SH coefficients; `shs` differs between the packages")
            if f.get("sh_degree", 0) != first.get("sh_degree", 0):
                raise ValueError(f"render_views: `sh_degree` differs between the packages ({first.get('sh_degree', 0)} and {f.get('sh_degree', 0)})")
            for key in ("opacities", "opacity_logits", "rgb"):
                if (f.get(key) is None) != (first.get(key) is None):
                    raise ValueError(f"render_views: `{key}` is given in some packages of the batch and not in others")
        stack = lambda key: None if first.get(key) is None else torch.stack([f[key] for f in frames])
        # appearance: the same tensor in every package stays (P,.) (shared by the views, gradients summed); tensors that differ --
        # the ColorField configuration evaluates colour and opacity per frame -- are stacked to (k,P,.) (per-view appearance)
        same = lambda key: all(f.get(key) is first.get(key) for f in frames)
        look = {key: first.get(key) if same(key) else stack(key) for key in ("opacities", "opacity_logits", "rgb")}
        pkg = dict(first, means3D=stack("means3D"), cov3D_precomp=stack("cov3D_precomp"), scales=stack("scales"), rotations=stack("rotations"),
                   **look)
    means3D = pkg["means3D"]
    if cameras is None:
        sizes = {(int(b["width"]), int(b["height"])) for b in batches}
        if len(sizes) == 1 and not any(is_cropped(b) for b in batches):
            cameras = CameraBatch(len(batches), int(batches[0]["width"]), int(batches[0]["height"]), device=means3D.device).set(batches)
        else:                        # cropped / mixed raster sizes: every view's crop window (all must paste to one W x H)
            W, H = crop_window(batches[0])[4:]
            for v, b in enumerate(batches):
                if crop_window(b)[4:] != (W, H):
                    raise ValueError(f"render_views: view {v}'s crop pastes to {crop_window(b)[4]}x{crop_window(b)[5]}, view 0's to {W}x{H} "
                                     "-- the views of a batch share one pasted image size")
            cameras = CameraBatch(len(batches), W, H, device=means3D.device, windowed=True).set(batches)
    opacities, act = pkg.get("opacities"), None
    if opacities is None and pkg.get("opacity_logits") is not None:
        opacities, act = pkg["opacity_logits"], "sigmoid"
    shs = pkg["shs"]
    out = rasterize_gaussians_views(means3D, shs, None if shs is not None else pkg["rgb"], opacities, pkg.get("scales"),
                                    pkg.get("rotations"), pkg.get("cov3D_precomp"), cameras, bg_color,
                                    sh_degree=pkg["sh_degree"] if "sh_degree" in pkg else 0, opacity_activation=act, l1_targets=targets,
                                    colors2=colors2, bg2=bg_color2, grad_sync=grad_sync, tile_cull=tile_cull)
    if colors2 is not None:
        return {"render": out[0], "render2": out[2]}
    return {"render": out[0], "l1": out[2]} if targets is not None else {"render": out[0]}


def render(batch, pkg, bg_color, colors_precomp=None, measure_time=False, solid_bg=True, fast=False, detach=[],
           grad_sync=None, _pair=None, _l1=None, crop_window=False):
    """crop_window (extension): with an off-centre crop (lib/batch.py:186-198) rasterize the pasted W x H window directly
    (include/d3ga.h: D3GA_CAMERA_SLOT_WINDOWED) instead of the padded w x h raster followed by `paste` -- the same image bit for
    bit, the same radii, the same gradients up to the summation order of float atomics, without the padding pixels and the
    paste's copies.  A windowed `cameras.CameraSlot` in the batch always renders its window."""
    means3D = pkg["means3D"]
    # a cameras.CameraSlot in the batch: the camera is read from its static device buffer (graph-capturable step that
    # follows the trainer's camera-per-step, d3ga_amd/graph.py)
    slot = batch.get("camera_slot")
    crop = batch["crop"]
    windowed = (slot is not None and getattr(slot, "windowed", False)) or (crop_window and slot is None and is_cropped(batch))
    if windowed and grad_sync is not None:
        raise ValueError("render: grad_sync is not available with crop-window rendering")
    if windowed and slot is None:
        W, H = int(crop[4]), int(crop[5])
        mats, row = window_camera(batch, device=means3D.device)
        view, full, campos, tfx = mats[0:16].view(4, 4), mats[32:48].view(4, 4), row, CAMERA_SLOT_WINDOWED
    else:
        cam = slot or batch_to_camera(batch, device=means3D.device)
        W, H = (slot.image_width, slot.image_height) if windowed else (int(batch["width"]), int(batch["height"]))
        view, full, campos, tfx = cam.world_view_transform, cam.full_proj_transform, cam.camera_center, cam.tanfovx
    if windowed:
        crop = None                       # the rasterizer's output IS the window

    settings = GaussianRasterizationSettings(
        image_height=H,
        image_width=W,
        tanfovx=tfx,
        tanfovy=tfx if windowed else cam.tanfovy,
        bg=bg_color,
        scale_modifier=1.0,
        viewmatrix=view,
        projmatrix=full,
        sh_degree=pkg["sh_degree"] if "sh_degree" in pkg else 0,
        campos=campos,
        prefiltered=False,
        debug=False,
        antialiasing=False,
        tile_cull=True,                   # (extension) lists from the alpha >= 1/255 box: the same image from shorter lists
    )

    # what the rasterizer is handed (renderer.py:95-120): geometry as packaged; `detach` names inputs whose gradient is cut
    # ("position", "covariance", "opacity": the silhouette pass of models/trainer.py:104-110); the colour is the explicit
    # `colors_precomp` if given, else the package's SH coefficients, else its RGB
    geo = {k: pkg.get(k) for k in ("cov3D_precomp", "scales", "rotations", "opacities")}
    # extension: a package may carry the raw `opacity_logits` instead of activated `opacities` (models/cage_net.py:247
    # applies sigmoid in Python): the activation then runs inside the per-Gaussian kernels, forward and backward
    act = None
    if geo["opacities"] is None and pkg.get("opacity_logits") is not None:
        geo["opacities"], act = pkg["opacity_logits"], "sigmoid"
    cut = {"position": "means3D", "covariance": "cov3D_precomp", "opacity": "opacities"}
    geo["means3D"] = means3D
    for name in detach:
        if name in cut:
            geo[cut[name]] = geo[cut[name]].detach()
    means3D, cov3D_precomp, scales, rotations, opacities = (geo[k] for k in ("means3D", "cov3D_precomp", "scales", "rotations", "opacities"))
    shs = pkg["shs"] if colors_precomp is None else None
    if colors_precomp is None and shs is None:
        colors_precomp = pkg["rgb"]

    # screen-space points: a zero tensor whose .grad receives dL/d(mean2D) (renderer.py:122-128).  A fresh leaf over a
    # cached block of zeros: no fill kernel per render (the rasterizer never reads or writes its values)
    means2D = _zero_leaf(means3D)
    # render fusion: when means3D and the covariance are the outputs of one cage-deform node, that node's per-Gaussian backward
    # runs inside the rasterizer's (cage_deform.claim_for_render states the conditions; one render per node and forward pass)
    node = None
    if grad_sync is None and not windowed and scales is None and rotations is None:
        from .cage_deform import claim_for_render
        node = claim_for_render(means3D, cov3D_precomp)
        node = node if node[0] is not None else None
    try:
        means2D.retain_grad()
    except Exception:
        pass

    if _pair is not None:
        img, _radii, _invd, img2 = rasterize_gaussians_pair(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                                            cov3D_precomp, settings, _pair[0], _pair[1], grad_sync, act,
                                                            want_invdepth=False, deform_node=node)
        if crop is None:
            return {"render": img, "render2": img2}
        return {"render": paste(img, crop), "render2": paste(img2, crop)}
    if _l1 is not None:
        img, _radii, _invd, loss = rasterize_gaussians_l1(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                                          cov3D_precomp, settings, _l1, grad_sync, act, want_invdepth=False,
                                                          deform_node=node)
        return {"render": img, "l1": loss}
    # the operator behind upstream's `GaussianRasterizer(raster_settings)(...)` module call (renderer.py:130-141), without
    # building an nn.Module per render: its constructor and attribute writes cost ~25 us of host time per call, a sixth of an
    # eager render's enqueue time (tools/prof_host.py); the module class stays available for callers that use it themselves
    if measure_time:
        torch.cuda.synchronize()
    rendered = rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, settings,
                                   grad_sync, act, want_invdepth=False, deform_node=node)[0]     # only [0] of the rasterizer's outputs is used here (renderer.py:141)
    if measure_time:
        torch.cuda.synchronize()
    return {"render": rendered if crop is None else paste(rendered, crop)}
