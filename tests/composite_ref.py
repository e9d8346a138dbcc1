"""CPU side of tests/test_gpu_composite_paths.py: the scenes, the C oracle's renders and backwards of them (oracle.raster_c), the
path tables, and a Python mirror of the two dispatches that pick a template instantiation of the compositing kernels
  forward   composite_fwd_q_kernel<DUAL, DEPTH, L1V, PVB, WIN>      (d3ga_amd/csrc/raster_composite.hip:450-463)
  backward  composite_bwd_tile_kernel<DUAL, S, INVD, 1, PVB, WIN>   (d3ga_amd/csrc/raster_composite_scan.hip:619-635)
No GPU call in here; tests/test_composite_paths_host.py checks the tables and the scenes' preconditions from the oracle alone."""
import functools
import itertools

import numpy as np
import torch

from d3ga_amd import cameras
from oracle import raster_c as rc
from util import Parity, scene_inputs

# ------------------------------------------------------------------------------------------------------------------------
# the instantiations, written out by hand
# ------------------------------------------------------------------------------------------------------------------------
# forward: (mode, DEPTH, PVB, WIN); mode plain = <false, ., false>, pair = DUAL, l1 = L1V
ALL_FWD_INSTANCES = {
    ("plain", False, False, False), ("plain", False, False, True), ("plain", False, True, False), ("plain", False, True, True),
    ("plain", True, False, False), ("plain", True, False, True), ("plain", True, True, False), ("plain", True, True, True),
    ("pair", False, False, False), ("pair", False, False, True), ("pair", False, True, False), ("pair", False, True, True),
    ("pair", True, False, False), ("pair", True, False, True), ("pair", True, True, False), ("pair", True, True, True),
    ("l1", False, False, False), ("l1", False, False, True), ("l1", False, True, False), ("l1", False, True, True),
    ("l1", True, False, False), ("l1", True, False, True), ("l1", True, True, False), ("l1", True, True, True),
}
# backward: (mode, S, PVB, WIN); mode plain = <false, S, false>, pair = DUAL, depth = INVD
ALL_BWD_INSTANCES = {
    ("plain", 256, False, False), ("plain", 256, False, True), ("plain", 256, True, False), ("plain", 256, True, True),
    ("plain", 512, False, False), ("plain", 512, False, True), ("plain", 512, True, False), ("plain", 512, True, True),
    ("pair", 256, False, False), ("pair", 256, False, True), ("pair", 256, True, False), ("pair", 256, True, True),
    ("pair", 512, False, False), ("pair", 512, False, True), ("pair", 512, True, False), ("pair", 512, True, True),
    ("depth", 256, False, False), ("depth", 256, False, True), ("depth", 256, True, False), ("depth", 256, True, True),
    ("depth", 512, False, False), ("depth", 512, False, True), ("depth", 512, True, False), ("depth", 512, True, True),
}

VARIANTS = (0, 32, 128, 160)             # composite_variant: bit 5 work-ordered dispatch, bit 7 exact block culling (default 160)
MERGE_SLOTS = (256, 512)                 # (default 512)
TILE_ASSIGN = (0, 1, 2, 10)              # 0 quadrants, 1 interleaved, 2 by list length (default), 10 = 2 + 8: no early exit
BWD_SPLIT = (-1, 0, 3)                   # -1 (default) the order kernel's count, 0 none, 3 the three heaviest tiles
FWD_TARGET = ("none", "target", "cell")  # the L1 target of d3ga_raster_composite_fwd_l1: absent, a pointer, a device cell
# the incoming gradient of a backward call: dL_dpix alone; the fused L1 source through `target` or `target_cell`, alone
# (dL_dpix == NULL) or with dL_dpix; dL_dinvdepth alone (dL_dpix == NULL) or with dL_dpix
BWD_SRC = ("dpix", "l1t", "l1c", "l1t+dpix", "l1c+dpix", "invd", "dpix+invd")
DEFAULT_KNOBS = dict(variant=160, slots=512, assign=2, split=-1)


def fwd_instance(colors2, partials, out_invdepth, n_views, per_view_background, windowed):
    """composite_fwd_impl's choice (raster_composite.hip:450-463) from the arguments of a call -> (mode, DEPTH, PVB, WIN);
    None: D3GA_E_CONFIG (colors2 together with the L1 partials, line 460)."""
    pvb = n_views > 1 and bool(per_view_background)                       # line 449
    if colors2 and partials:
        return None                                                      # line 460
    mode = "pair" if colors2 else ("l1" if partials else "plain")        # lines 461-463
    return (mode, bool(out_invdepth), pvb, bool(windowed))               # lines 456-458: WIN, PVB


def bwd_instance(colors2, dL_dinvd, merge_slots, n_views, per_view_background, windowed):
    """launch_composite_bwd_scan's choice (raster_composite_scan.hip:619-635) -> (mode, S, PVB, WIN); None: D3GA_E_CONFIG
    (dL_dinvdepth together with colors2, line 631)."""
    pvb = n_views > 1 and bool(per_view_background)                       # line 616
    S = 512 if merge_slots >= 512 else 256                               # lines 632-635
    if dL_dinvd:
        if colors2:
            return None                                                  # line 631
        return ("depth", S, pvb, bool(windowed))                         # line 632
    return ("pair" if colors2 else "plain", S, pvb, bool(windowed))      # lines 633-635


def row_fwd_instance(r):
    return fwd_instance(r["mode"] == "pair", r["mode"] == "l1", r["depth"], r["k"], r["pvb"], r["window"])


def row_bwd_instance(r):
    return bwd_instance(r["mode"] == "pair", "invd" in r["src"], r["slots"], r["k"], r["pvb"], r["window"])


# ------------------------------------------------------------------------------------------------------------------------
# the tables: every instantiation first, then rows until every feasible pair of factor values meets in some row
# ------------------------------------------------------------------------------------------------------------------------
def fwd_feasible(fa, a, fb, b):
    """A pair of factor values that some call can have: the L1 target exists on the l1 rows and only there."""
    pair = {fa: a, fb: b}
    if "mode" in pair and "target" in pair:
        return (pair["mode"] == "l1") == (pair["target"] != "none")
    return True


def bwd_feasible(fa, a, fb, b):
    """The fused L1 source and the inverse-depth gradient are single-image launches: src l1* on the plain instantiations, src
    *invd = mode depth, the pair takes dL_dpix (and dL_dpix2)."""
    pair = {fa: a, fb: b}
    if "mode" in pair and "src" in pair:
        m, s = pair["mode"], pair["src"]
        return (m == "depth") == ("invd" in s) and (m != "pair" or s == "dpix")
    return True


def pairs_missing(rows, factors, feasible):
    """mlp_ref.pairs_missing with a feasibility rule: the feasible pairs of values (of two different factors) that no row has."""
    missing = []
    for (fa, va), (fb, vb) in itertools.combinations(factors.items(), 2):
        have = {(r[fa], r[fb]) for r in rows}
        missing += [(fa, a, fb, b) for a in va for b in vb if feasible(fa, a, fb, b) and (a, b) not in have]
    return missing


def _cover(candidates, factors, feasible, inst_of, instances, fixed=()):
    """Deterministic greedy cover: per instantiation the candidate that adds the most uncovered pairs (rotating the start so that
    ties do not always fall on the first value), then candidates until no feasible pair is missing."""
    names = list(factors)
    want = {(fa, a, fb, b) for (fa, va), (fb, vb) in itertools.combinations(factors.items(), 2) for a in va for b in vb
            if feasible(fa, a, fb, b)}

    def pairs_of(r):
        return {(fa, r[fa], fb, r[fb]) for fa, fb in itertools.combinations(names, 2)}
    rows, covered = list(fixed), set()
    for r in rows:
        covered |= pairs_of(r)
    step = 0

    def best(pool):
        nonlocal step
        n = len(pool)
        order = [pool[(7 * step + 13 * i) % n] for i in range(n)] if n % 13 and n % 7 else pool
        step += 1
        return max(order, key=lambda c: len((pairs_of(c) & want) - covered))
    have = {inst_of(r) for r in rows}
    for inst in sorted(instances, key=repr):
        if inst in have:
            continue
        c = best([c for c in candidates if inst_of(c) == inst])
        rows.append(c)
        covered |= pairs_of(c)
    while (want - covered):
        c = best(candidates)
        assert (pairs_of(c) & want) - covered, "no candidate covers a missing pair"
        rows.append(c)
        covered |= pairs_of(c)
    return rows


FWD_FACTORS = dict(mode=("plain", "pair", "l1"), depth=(False, True), pvb=(False, True), window=(False, True), variant=VARIANTS,
                   forward_only=(False, True), target=FWD_TARGET)
BWD_FACTORS = dict(mode=("plain", "pair", "depth"), pvb=(False, True), window=(False, True), variant=VARIANTS, slots=MERGE_SLOTS,
                   assign=TILE_ASSIGN, split=BWD_SPLIT, src=BWD_SRC)


def _set_name(scene, k, window):
    return f"{scene}{'w' if window else ''}{k}"


def fwd_table():
    """Rows of the forward table: dicts with the factors of FWD_FACTORS, k (views: 2 with per-view backgrounds, else 1 or 2 by
    turns), the camera set, the instantiation and an id."""
    cands = []
    for mode, depth, pvb, window, variant, fo in itertools.product(*(FWD_FACTORS[f] for f in ("mode", "depth", "pvb", "window", "variant", "forward_only"))):
        for target in (("target", "cell") if mode == "l1" else ("none",)):
            cands.append(dict(mode=mode, depth=depth, pvb=pvb, window=window, variant=variant, forward_only=fo, target=target))
    for c in cands:
        c["k"] = 2 if c["pvb"] else 1                # (provisional: the instantiation does not depend on k without pvb)
    rows = _cover(cands, FWD_FACTORS, fwd_feasible, row_fwd_instance, ALL_FWD_INSTANCES)
    out = []
    for i, r in enumerate(rows):
        r = dict(r)
        r["k"] = 2 if (r["pvb"] or i % 3 == 2) else 1                     # a shared background over two views on every third row
        r["scene"], r["set"], r["inst"] = "small", _set_name("small", r["k"], r["window"]), row_fwd_instance(r)
        r["id"] = (f"{i:02d}_{r['mode']}{'_depth' if r['depth'] else ''}{'_pvb' if r['pvb'] else ''}{'_win' if r['window'] else ''}_k{r['k']}"
                   f"_v{r['variant']}{'_fo' if r['forward_only'] else ''}{'' if r['target'] == 'none' else '_' + r['target']}")
        out.append(r)
    return out


# the rows on the `deep` scene (one view, no window): both cache sizes, the three modes, tile_assign 0, 1, 2 (and 10), bwd_split 0, 3
_DEEP_ROWS = [
    dict(mode="plain", src="dpix", slots=512, assign=2, split=-1, variant=160),
    dict(mode="plain", src="dpix", slots=256, assign=0, split=0, variant=160),
    dict(mode="pair", src="dpix", slots=512, assign=1, split=3, variant=160),
    dict(mode="pair", src="dpix", slots=256, assign=2, split=-1, variant=32),
    dict(mode="depth", src="dpix+invd", slots=512, assign=0, split=3, variant=32),
    dict(mode="depth", src="invd", slots=256, assign=1, split=0, variant=128),
    dict(mode="plain", src="l1t+dpix", slots=256, assign=10, split=3, variant=160),
    dict(mode="plain", src="dpix", slots=512, assign=1, split=0, variant=0),
    dict(mode="depth", src="dpix+invd", slots=256, assign=2, split=3, variant=160),
]


def bwd_table():
    """Rows of the backward table: the `deep` rows above, then rows on the `small` scene until all 24 instantiations are reached
    and no feasible pair of BWD_FACTORS is missing."""
    fixed = [dict(r, pvb=False, window=False, k=1, scene="deep") for r in _DEEP_ROWS]
    # the `small` scene under the library's defaults, one row per mode (full raster, shared background)
    fixed += [dict(mode=m, src=s, pvb=False, window=False, k=1, scene="small", slots=512, assign=2, split=-1, variant=160)
              for m, s in (("plain", "dpix"), ("pair", "dpix"), ("depth", "dpix+invd"))]
    cands = []
    for mode, pvb, window, variant, slots, assign, split in itertools.product(*(BWD_FACTORS[f] for f in ("mode", "pvb", "window", "variant", "slots", "assign", "split"))):
        for src in [s for s in BWD_SRC if bwd_feasible("mode", mode, "src", s)]:
            cands.append(dict(mode=mode, pvb=pvb, window=window, variant=variant, slots=slots, assign=assign, split=split, src=src,
                              k=2 if pvb else 1, scene="small"))
    rows = _cover(cands, BWD_FACTORS, bwd_feasible, row_bwd_instance, ALL_BWD_INSTANCES, fixed)
    out = []
    for i, r in enumerate(rows):
        r = dict(r)
        if r["scene"] == "small":
            r["k"] = 2 if (r["pvb"] or i % 3 == 2) else 1
        r["set"], r["inst"] = _set_name(r["scene"], r["k"], r["window"]), row_bwd_instance(r)
        r["id"] = (f"{i:02d}_{r['scene']}_{r['mode']}_{r['src']}{'_pvb' if r['pvb'] else ''}{'_win' if r['window'] else ''}_k{r['k']}"
                   f"_S{r['slots']}_a{r['assign']}_s{r['split']}_v{r['variant']}")
        out.append(r)
    return out


def is_default_knobs(r):
    return all(r.get(k, v) == v for k, v in DEFAULT_KNOBS.items())


# ------------------------------------------------------------------------------------------------------------------------
# scenes
# ------------------------------------------------------------------------------------------------------------------------
BG0, BG1, BG2 = (0.3, 0.6, 0.1), (0.9, 0.2, 0.5), (0.1, 0.05, 0.2)     # shared / view 1's own / the pair's second background
WIN_W, WIN_H = 37, 29
# principal points of the windowed views: those of CROPS[2] and CROPS[3] of tests/test_gpu_crop_window.py ((197, 150, 120, 53),
# (203, 149, 80, 101)) scaled to the 37 x 29 window -- the window at the left / bottom and at the right / top of its padded
# raster, offsets 9 and 7 (no multiple of 8: quadrants fall partly, and with the spare tile row and column wholly, outside)
WIN_PP = ((23, 10), (15, 20))
AZIMUTHS = (0.4, 1.3)
DEEP = dict(N=1400, spread=0.15, sigma=0.05, op_lo=0.008, op_hi=0.016, seed=5)


@functools.lru_cache(maxsize=None)
def gaussians(scene):
    """-> dict of float32 CPU tensors: means3D (P,3), cov6 (P,6), opacities (P,), rgb (P,3), colors2 (P,3)."""
    if scene == "small":
        inp = scene_inputs("T0", scale_mult=3.0)
        g = dict(means3D=inp["means3D"], cov6=inp["cov6"], opacities=inp["opacities"].reshape(-1).contiguous(), rgb=inp["rgb"].contiguous())
        gen = torch.Generator().manual_seed(11)
    else:
        inp = scene_inputs("T0", width=32, height=32)
        d = DEEP
        gen = torch.Generator().manual_seed(d["seed"])
        N = d["N"]
        means = inp["means3D"].mean(0, keepdim=True) + d["spread"] * torch.randn(N, 3, generator=gen)
        sig = d["sigma"] * (0.5 + torch.rand(N, 3, generator=gen))
        cov6 = torch.zeros(N, 6)
        cov6[:, 0], cov6[:, 3], cov6[:, 5] = sig[:, 0] ** 2, sig[:, 1] ** 2, sig[:, 2] ** 2
        op = d["op_lo"] + (d["op_hi"] - d["op_lo"]) * torch.rand(N, generator=gen)
        g = dict(means3D=means.contiguous(), cov6=cov6, opacities=op, rgb=torch.rand(N, 3, generator=gen))
    g["colors2"] = torch.rand(g["means3D"].shape[0], 3, generator=gen)
    return {k: v.float().contiguous() for k, v in g.items()}


class View:
    """One camera of a set: the oracle's raster (w x h), the image the kernels write (W x H: the raster, or the window at (ox, oy)
    of it), and the numbers the device needs."""

    def __init__(self, scene, azimuth, pp=None):
        if scene == "deep":
            inp = scene_inputs("T0", width=32, height=32, azimuth=azimuth)
        elif pp is None:
            inp = scene_inputs("T0", scale_mult=3.0, azimuth=azimuth)
        else:
            inp = scene_inputs("T0", scale_mult=3.0, azimuth=azimuth, width=WIN_W, height=WIN_H, cx=pp[0], cy=pp[1])
        self.batch, self.cam, self.windowed = inp["batch"], inp["cam"], pp is not None
        self.w, self.h = int(inp["W"]), int(inp["H"])
        if self.windowed:
            w, h, self.ox, self.oy, self.W, self.H = cameras.crop_window(self.batch)
            assert (w, h) == (self.w, self.h) and (self.W, self.H) == (WIN_W, WIN_H)
        else:
            self.ox, self.oy, self.W, self.H = 0, 0, self.w, self.h
        self.view = np.asarray(self.cam["world_view_transform"], np.float32).reshape(16)
        self.proj = np.asarray(self.cam["full_proj_transform"], np.float32).reshape(16)
        self.campos = np.asarray(self.cam["camera_center"], np.float32).reshape(3)

    def crop(self, a):
        """The window of an array whose last two axes are the raster."""
        return a[..., self.oy:self.oy + self.H, self.ox:self.ox + self.W]

    def embed(self, a):
        """A window image (.., H, W) in a raster of zeros (.., h, w): an incoming gradient as the full-raster oracle takes it."""
        if a is None:
            return None
        a = np.asarray(a, np.float32)
        out = np.zeros(a.shape[:-2] + (self.h, self.w), np.float32)
        out[..., self.oy:self.oy + self.H, self.ox:self.ox + self.W] = a
        return out

    def window_row(self):
        """The 9 floats of the windowed camera row (include/d3ga.h: D3GA_CAMERA_SLOT_WINDOWED)."""
        return cameras.window_row_host(self.batch)[48:57].copy()


SETS = {"small1": ("small", 1, False), "small2": ("small", 2, False), "smallw1": ("small", 1, True), "smallw2": ("small", 2, True),
        "deep1": ("deep", 1, False)}


@functools.lru_cache(maxsize=None)
def views(set_name):
    scene, k, window = SETS[set_name]
    return tuple(View(scene, AZIMUTHS[v], WIN_PP[v] if window else None) for v in range(k))


def background(pvb, v):
    return BG1 if (pvb and v == 1) else BG0


class Render:
    """The oracle's render of one view over one background: colour and inverse depth cut to the image the kernels write, the
    context for the backward, and the marginal pixels of that image (util.Parity, its pixel mask cut to the window)."""

    def __init__(self, set_name, v, bg, second):
        vw, g = views(set_name)[v], gaussians(SETS[set_name][0])
        col, self.radii, invd, self.ctx = rc.forward(
            g["means3D"].numpy(), g["opacities"].numpy(), np.asarray(bg, np.float32), vw.cam["world_view_transform"], vw.cam["full_proj_transform"],
            vw.cam["camera_center"], vw.cam["tanfovx"], vw.cam["tanfovy"], vw.w, vw.h, cov3D_precomp=g["cov6"].numpy(),
            colors_precomp=(g["colors2"] if second else g["rgb"]).numpy())
        self.full_color = col
        self.color, self.invd = vw.crop(col).copy(), vw.crop(invd).copy()
        self.par = Parity(self.ctx)
        self.par_full_pix = self.par.pix
        self.par.pix = vw.crop(self.par.pix).copy()          # Parity.image / .mask on W x H images
        self.pix = self.par.pix


@functools.lru_cache(maxsize=None)
def render(set_name, v, bg=BG0, second=False):
    return Render(set_name, v, bg, second)


def row_renders(set_name, pvb, second=False):
    """The oracle renders of a row's views: view v over background(pvb, v), or (second) the pair's image over BG2."""
    return [render(set_name, v, BG2 if second else background(pvb, v), second) for v in range(len(views(set_name)))]


@functools.lru_cache(maxsize=None)
def incoming(set_name, pvb):
    """The incoming gradients and the L1 target of a camera set, float32 numpy, one block per view: gpix, gpix2 (k,3,H,W), gd
    (k,H,W), target (k,3,H,W), g_loss; pix (k,H,W) the oracle's marginal pixels, on which gpix, gpix2 and gd are zero (the masked
    protocol of util.Parity).  The target keeps 1e-3 away from the oracle's image, so that sign(image - target) is the same for
    every image within the image bar; g_loss is sized so that the L1 term of dL/dpixel is 0.5 sign(.), next to a unit normal
    dL_dpix."""
    vs = views(set_name)
    k, W, H = len(vs), vs[0].W, vs[0].H
    gen = torch.Generator().manual_seed(100 + sum(map(ord, set_name)))
    gpix, gpix2 = torch.randn(k, 3, H, W, generator=gen).numpy(), torch.randn(k, 3, H, W, generator=gen).numpy()
    gd, target = torch.randn(k, H, W, generator=gen).numpy(), torch.rand(k, 3, H, W, generator=gen).numpy()
    rs = row_renders(set_name, pvb)
    pix = np.stack([r.pix for r in rs])
    for v, r in enumerate(rs):
        gpix[v][:, r.pix] = 0
        gpix2[v][:, r.pix] = 0
        gd[v][r.pix] = 0
        d = r.color.astype(np.float64) - target[v]
        near = np.abs(d) < 1e-3
        target[v][near] = (r.color[near] + np.where(d[near] >= 0, -2e-3, 2e-3)).astype(np.float32)
        assert (np.abs(r.color.astype(np.float64) - target[v]) >= 1e-3).all()
    return dict(gpix=gpix, gpix2=gpix2, gd=gd, target=target, pix=pix, g_loss=np.float32(0.5 * 3 * W * H * k))


GRAD_KEYS = ("means3D", "cov3D", "opacities", "colors")


@functools.lru_cache(maxsize=None)
def oracle_gradients(set_name, pvb, mode, src, with_noise=False):
    """The oracle's gradients of a backward row, summed over the views as d3ga_raster_preprocess_bwd sums them ->
    ({means3D, cov3D, opacities, colors} float64, the same keys' conditioning noise or None).
    Incoming gradient per view: dL_dpix where src has it, + g_loss / (3 W H k) sign(image - target) for an L1 source (zero on
    the marginal pixels), dL_dinvdepth for *invd; a pair row adds the backward of the second render under gpix2, without that
    render's colour gradient (colors2 are constants)."""
    inc, vs = incoming(set_name, pvb), views(set_name)
    k, W, H = len(vs), vs[0].W, vs[0].H
    total = noise = None
    for v, (vw, r) in enumerate(zip(vs, row_renders(set_name, pvb))):
        gp = inc["gpix"][v].astype(np.float64) if "dpix" in src else np.zeros((3, H, W))
        if src.startswith("l1"):
            sgn = np.sign(r.color.astype(np.float64) - inc["target"][v])
            sgn[:, r.pix] = 0
            gp = gp + float(inc["g_loss"]) / (3.0 * W * H * k) * sgn
        gd = vw.embed(inc["gd"][v]) if "invd" in src else None
        calls = [(r.ctx, vw.embed(gp), gd, GRAD_KEYS)]
        if mode == "pair":
            calls.append((render(set_name, v, BG2, True).ctx, vw.embed(inc["gpix2"][v]), None, GRAD_KEYS[:3]))
        for ctx, g_in, g_d, keys in calls:
            og = rc.backward(ctx, g_in, dL_dinvdepth=g_d)
            part = {key: (np.asarray(og[key], np.float64) if key in keys else 0.0) for key in GRAD_KEYS}
            total = part if total is None else {key: total[key] + part[key] for key in GRAD_KEYS}
            if with_noise:
                nz = sum_noise(ctx, g_in, g_d, og, keys)
                noise = nz if noise is None else {key: noise[key] + nz[key] for key in GRAD_KEYS}
    total = {key: np.asarray(val, np.float64).reshape(len(total["means3D"]), -1) for key, val in total.items()}
    return total, noise


def sum_noise(ctx, gpix, gd, grads, keys):
    """util.conditioning_noise (the exact first-order worst case over the 13 probes, gamma = util.SUM_NOISE_GAMMA) with the
    inverse-depth gradient passed along: what float32 accumulation of the per-Gaussian pixel sums does to each element."""
    from util import SUM_NOISE_GAMMA
    out = {key: 0.0 for key in GRAD_KEYS}
    for pat in range(1000, 1013):
        g2 = rc.backward(ctx, gpix, sum_noise=(SUM_NOISE_GAMMA, pat), dL_dinvdepth=gd)
        for key in keys:
            out[key] = out[key] + 2.0 * np.abs(np.asarray(g2[key], np.float64) - np.asarray(grads[key], np.float64))
    return out


def grad_excess(mine, ref, noise=None, rtol=1e-3, atol_rel=1e-6):
    """The strict bar of util.Parity.grads on every Gaussian (the incoming gradients are masked): the worst
    |a - b| / (1e-3 |b| + 1e-6 max|b| (+ noise)); <= 1 passes."""
    b = np.asarray(ref, np.float64)
    a = np.asarray(mine, np.float64).reshape(b.shape)
    assert np.isfinite(a).all()
    allow = rtol * np.abs(b) + atol_rel * (np.abs(b).max() + 1e-300)
    if noise is not None:
        allow = allow + np.asarray(noise, np.float64).reshape(b.shape)
    return float((np.abs(a - b) / allow).max())


# ------------------------------------------------------------------------------------------------------------------------
# the `deep` scene's preconditions, from the oracle alone
# ------------------------------------------------------------------------------------------------------------------------
def deep_facts():
    """-> dict: min final_T, marginal pixels, pixels, per tile the list length and the number of entries with alpha >= 1/255 on
    at least one pixel of the tile (float64, from rc.geom's xy and conic_o; entries within 1e-5 of the threshold left out), and
    the number of Gaussians with a non-zero opacity gradient under the set's dL_dpix."""
    r = render("deep1", 0)
    vw = views("deep1")[0]
    ge = rc.geom(r.ctx)
    start, plist = rc.tile_lists(r.ctx)
    xy, co = ge["xy"].astype(np.float64), ge["conic_o"].astype(np.float64)
    gx = (vw.w + 15) // 16
    lens, alive = [], []
    for t in range(len(start) - 1):
        ids = plist[start[t]:start[t + 1]]
        px = (t % gx) * 16 + np.arange(16, dtype=np.float64)
        py = (t // gx) * 16 + np.arange(16, dtype=np.float64)
        dx = xy[ids, 0][:, None, None] - px[None, None, :]
        dy = xy[ids, 1][:, None, None] - py[None, :, None]
        power = -0.5 * (co[ids, 0][:, None, None] * dx * dx + co[ids, 2][:, None, None] * dy * dy) - co[ids, 1][:, None, None] * dx * dy
        alpha = np.where(power > 0, 0.0, np.minimum(0.99, co[ids, 3][:, None, None] * np.exp(np.minimum(power, 0.0))))
        inside = (px[None, None, :] < vw.w) & (py[None, :, None] < vw.h)
        amax = np.where(inside, alpha, 0.0).reshape(len(ids), -1).max(1) if len(ids) else np.zeros(0)
        lens.append(len(ids))
        alive.append(int((amax >= 1.0 / 255.0 + 1e-5).sum()))
    og = rc.backward(r.ctx, incoming("deep1", False)["gpix"][0])
    return dict(min_T=float(ge["final_T"].min()), marginal=int(r.pix.sum()), pixels=int(r.pix.size), lens=lens, alive=alive,
                with_opacity_grad=int((np.asarray(og["opacities"]).reshape(-1) != 0).sum()), P=len(xy))
