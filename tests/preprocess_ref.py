"""Float64 side of tests/test_preprocess_alone_host.py and tests/test_gpu_preprocess_alone.py: the per-Gaussian kernels
(d3ga_amd/csrc/raster_pre.hip, raster_pre_body.h: projection, SH colour, the R6 per-Gaussian backward) on their own, against
oracle/raster_torch.preprocess under float64 autograd.  CPU only.

  edge_scene   Gaussians built in camera space and mapped to the world: a table of named edge classes (CLASS_TABLE), the rest
               filled by a seeded sampler, the same rows in the same order for host and device.  Every decision the float32 code
               takes (near plane, radius, tile rectangle, guard band, antialiasing floor, colour clamp) is at a distance from its
               threshold in the float64 reference, in every camera of the scene: the builder draws again otherwise, and asserts it.
  reference    the protocol of tests/test_hostcheck_math.py::_bwd_case: a hand-made accumulator `acc`, and autograd through
               oracle/raster_torch.preprocess of the linear functional it stands for, summed over the rows the float64 forward
               calls visible.  One thing is restated on top of autograd: the backward's guarded denominator (_GuardedDenominator).
  bars         per output e32 = the worst row error of the float32 CPU evaluation of the same reference against the float64 one,
               relative to the row's largest element, floored at 2^-22; a class of at least four visible rows is held to the e32
               of its own rows.  A tested output D passes when on every row
               max_j |D[i,j] - G[i,j]| <= 4 e32 max_j |G[i,j]|  (the margin of tests/test_gpu_perceptual.py: same precision,
               another order of operations, contraction).
  check_grads  the bars, and what must hold exactly: culled rows, clamped channels, SH coefficients above the active degree and
               dL_dmeans2D[:, 2] are zeros; dL_dmeans2D[:, :2] is acc[:, :2]; without antialiasing and with the identity
               activation dL_dopacity is acc[:, 6]."""
import math

import numpy as np
import torch

from oracle import camera as ocam
from oracle import raster_torch as rt

W, H = 64, 48
TANX, TANY = 0.5, 0.375                  # focal length 64 pixels on both axes
NEAR, AA_FLOOR, DILATE = 0.2, 0.000025, 0.3
MARGIN = 4.0
E32_FLOOR = 2.0 ** -22
ACC_STRIDE = 16                          # D3GA_ACC_STRIDE

# class -> kinds (each drawn by _draw); COUNT of each kind in a full table.  A class holds >= 8 rows where P allows.
CLASS_TABLE = (
    ("plain", ("plain_axis", "plain_off", "plain_aniso"), (2, 3, 3)),
    ("guard", ("guard_x", "guard_y", "guard_xy"), (3, 3, 3)),
    ("tiny", ("tiny_below", "tiny_above"), (4, 4)),
    ("huge", ("huge",), (8,)),
    ("near", ("near_in", "near_out"), (4, 4)),
    ("culled", ("behind", "offscreen", "nan_opacity"), (3, 3, 3)),
    ("clamp", ("clamp_0", "clamp_12", "clamp_012"), (3, 3, 3)),
    ("rotation", ("rot_05", "rot_10", "rot_17"), (3, 3, 3)),
)
KIND_CLASS = {k: c for c, kinds, _ in CLASS_TABLE for k in kinds}
TABLE_ROWS = sum(sum(n) for _, _, n in CLASS_TABLE)          # 68


class Cfg:
    """One configuration of the kernels: colour path (M, deg; M = 0: precomputed colours), covariance path, switches."""

    def __init__(self, M=16, deg=3, from_sr=False, mod=1.0, aa=False, sigmoid=False, window=None):
        """window = (w, h, ox, oy): a windowed camera slot -- the W x H raster is the window at (ox, oy) of a w x h raster with the
        same focal length, i.e. a camera with an off-centre principal point."""
        self.M, self.deg, self.from_sr, self.mod, self.aa, self.sigmoid = M, deg, from_sr, float(np.float32(mod)), aa, sigmoid
        self.W, self.H, self.window = W, H, window
        self.Wr, self.Hr = (window[0], window[1]) if window else (W, H)              # the raster the camera projects on
        self.tanx, self.tany = float(np.float32(TANX * self.Wr / W)), float(np.float32(TANY * self.Hr / H))

    @property
    def sh(self):
        return self.M > 0

    def __repr__(self):
        col = f"sh M={self.M} deg={self.deg}" if self.sh else "colours"
        cov = f"scale/rot x{self.mod:g}" if self.from_sr else "cov6"
        return f"{col}, {cov}, aa={int(self.aa)}, sigmoid={int(self.sigmoid)}" + (f", window {self.window}" if self.window else "")


# ----------------------------------------------------------------------------------------------------------------------------
# cameras
# ----------------------------------------------------------------------------------------------------------------------------
def _rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K


R0 = _rot([0.3, -0.8, 0.52], 0.7)        # view 0: a generic rotation, so that every entry of the view matrix takes part
T0 = np.array([0.15, -0.1, 0.3])
CENTRE_CAM = np.array([0.0, 0.0, 2.0])   # where the scene sits in view 0's camera space


def cameras(k, cfg):
    """k cameras (oracle.camera dicts) around the scene: view 0 is the one the classes are defined in."""
    fovx, fovy = 2 * math.atan(cfg.tanx), 2 * math.atan(cfg.tany)
    c_world = R0 @ (CENTRE_CAM - T0)                       # p_view = R^T p + T
    cams = []
    for v in range(k):
        R = R0 @ _rot([0.2, 1.0, -0.1], 0.23 * v) @ _rot([1.0, 0.1, 0.3], -0.11 * v)
        T = T0 if v == 0 else np.array([0.05 * v, -0.03 * v, 2.0 + 0.07 * v]) - R.T @ c_world
        cams.append(ocam.camera(R, T, fovx, fovy))
    return cams


def cam_arrays(cam):
    return (np.ascontiguousarray(cam["world_view_transform"], np.float32), np.ascontiguousarray(cam["full_proj_transform"], np.float32),
            np.ascontiguousarray(cam["camera_center"], np.float32))


# ----------------------------------------------------------------------------------------------------------------------------
# the builder
# ----------------------------------------------------------------------------------------------------------------------------
def _unit_quats(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _draw(kind, n, rng, cfg):
    """n candidates of one kind -> camera-space means, scales (before the modifier), quaternions, opacities, SH rows."""
    f = cfg.Wr / (2 * cfg.tanx)                                  # pixels per unit of x/z
    u = lambda lo, hi, *s: rng.uniform(lo, hi, size=(n,) + s)
    z = u(1.2, 3.0)
    xz, yz = u(-0.85, 0.85) * cfg.tanx, u(-0.85, 0.85) * cfg.tany
    s = np.exp(u(math.log(0.02), math.log(0.15), 3))
    q = _unit_quats(rng, n)
    # at most 0.8: under the sigmoid activation dL/dlogit = g s (1 - s), and 1 - s carries the rounding of s amplified by s / (1 - s)
    # (19 at 0.95) in every class alike, so that a class's e32, taken over a few rows, meets it only by chance
    op = u(0.1, 0.8)
    sh = 0.25 * rng.normal(size=(n, 16, 3))
    sh[:, 0] += 0.8                                                # bright: no channel clamps unless the kind says so
    if kind == "plain_axis":
        xz, yz = 0.0 * xz, 0.0 * yz
    elif kind == "plain_aniso":                                    # scale ratios up to 1e3
        s = np.stack([u(0.1, 0.3), u(0.1, 0.3) * 10.0 ** -u(1.0, 2.0), u(0.1, 0.3) * 10.0 ** -u(2.0, 3.0)], 1)
        s = np.take_along_axis(s, np.argsort(rng.random((n, 3)), 1), 1)
    elif kind in ("guard_x", "guard_y", "guard_xy"):               # outside 1.3 tanfov, wide enough to reach the raster
        sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
        if kind != "guard_y":
            xz = sign * u(1.35, 1.6) * cfg.tanx
        if kind != "guard_x":
            yz = sign * u(1.35, 1.6) * cfg.tany
        s = np.exp(u(math.log(0.25), math.log(0.45), 3))
    elif kind in ("tiny_below", "tiny_above"):                     # det(cov2D) / det(cov2D + 0.3 I) on either side of 2.5e-5
        lam = u(3e-4, 1.2e-3) if kind == "tiny_below" else u(1.6e-3, 2.0e-3)      # rho ~ lam^2 / 0.09: < 1.6e-5 | 2.8e-5 .. 4.4e-5
        xz, yz = 0.5 * xz, 0.5 * yz
        s = (np.sqrt(lam) * z / f)[:, None] * u(0.97, 1.03, 3) / cfg.mod
    elif kind == "huge":                                           # three sigma beyond the raster
        s = u(1.2, 2.5, 3) * (z / 2.0)[:, None]
    elif kind in ("near_in", "near_out"):
        z = NEAR + (1e-3 if kind == "near_in" else -1e-3) * u(0.9, 1.1)
        xz, yz = 0.5 * xz, 0.5 * yz
        s = np.exp(u(math.log(2e-3), math.log(8e-3), 3))
    elif kind == "behind":
        z = -u(0.3, 3.0)
    elif kind == "offscreen":                                      # the tile rectangle is empty
        xz = np.where(rng.random(n) < 0.5, -1.0, 1.0) * u(2.5, 4.0) * cfg.tanx
        s = np.exp(u(math.log(0.01), math.log(0.03), 3))
    elif kind == "nan_opacity":
        op = np.full(n, np.nan)
    elif kind.startswith("clamp_"):
        for c in kind[6:]:
            sh[:, 0, int(c)] = -u(2.2, 3.5)                         # SH_C0 * (-2.2) + 0.5 < 0
        sh[:, 1:] *= 0.3
    elif kind.startswith("rot_"):
        q = q * {"rot_05": 0.5, "rot_10": 1.0, "rot_17": 1.7}[kind]
        s = np.exp(u(math.log(0.05), math.log(0.2), 3))
    if kind not in ("rot_05", "rot_10", "rot_17"):
        q = q * u(0.8, 1.25)[:, None]                              # never exactly unit norm: the kernels take it as given
    mean_cam = np.stack([xz * z, yz * z, z], 1)
    return dict(mean_cam=mean_cam, scales=s, rotations=q, opacities=op, shs=sh)


def _assemble(parts, cfg):
    """Candidate dicts -> the float32 inputs the kernels get."""
    cat = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    means = (cat["mean_cam"] - T0) @ R0.T                          # world = R (p_view - T)
    sc = dict(means3D=means.astype(np.float32), scales=cat["scales"].astype(np.float32), rotations=cat["rotations"].astype(np.float32),
              opacities=cat["opacities"].astype(np.float32).reshape(-1, 1), shs=cat["shs"].astype(np.float32))
    s64, q64 = torch.from_numpy(sc["scales"]).double(), torch.from_numpy(sc["rotations"]).double()
    Mm = rt._quat_rot_nonorm(q64) * (cfg.mod * s64)[:, None, :]
    S = Mm @ Mm.transpose(1, 2)
    sc["cov6"] = torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).numpy().astype(np.float32)
    sc["rgb"] = np.clip(rt.SH_C0 * sc["shs"][:, 0] + 0.5, 0.0, None).astype(np.float32) + np.float32(0.05)     # precomputed colours
    op = sc["opacities"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        sc["logits"] = np.log(op / (1 - op)).astype(np.float32)
    return sc


def forward64(sc, cfg, cam, dtype=torch.float64):
    """The float64 forward of `sc` in one camera and every quantity a decision hangs on.  With cfg.window: projected on the w x h
    raster, visible only where the tile rectangle meets the W x H window's tiles (radii_full: the full raster's radii)."""
    window = cfg.window
    view, proj, campos = (torch.from_numpy(a) for a in cam_arrays(cam))
    t = lambda a: torch.from_numpy(a).to(dtype)
    Wr, Hr = cfg.Wr, cfg.Hr
    kw = dict(scales=t(sc["scales"]), rotations=t(sc["rotations"]), scale_modifier=cfg.mod) if cfg.from_sr else dict(cov3D_precomp=t(sc["cov6"]))
    kw.update(dict(shs=t(sc["shs"][:, :cfg.M]), sh_degree=cfg.deg) if cfg.sh else dict(colors_precomp=t(sc["rgb"])))
    op = torch.sigmoid(t(sc["logits"])) if cfg.sigmoid else t(sc["opacities"])
    with torch.no_grad():
        pre = rt.preprocess(t(sc["means3D"]), op, view, proj, campos, cfg.tanx, cfg.tany, Wr, Hr, antialiasing=cfg.aa, **kw)
        hom = torch.cat([t(sc["means3D"]), torch.ones(len(op), 1, dtype=dtype)], 1)
        pv = hom @ view.to(dtype)[:, :3]
        o = dict(z=pv[:, 2], xz=pv[:, 0] / pv[:, 2], yz=pv[:, 1] / pv[:, 2])
        cn = pre["conic"]
        det = 1.0 / (cn[:, 0] * cn[:, 2] - cn[:, 1] * cn[:, 1])
        a, b, c = cn[:, 2] * det, -cn[:, 1] * det, cn[:, 0] * det
        mid = 0.5 * (a + c)
        o["det"] = det
        o["r3"] = 3.0 * torch.sqrt(mid + torch.sqrt(torch.clamp(mid * mid - det, min=0.1)))
        o["rho"] = ((a - DILATE) * (c - DILATE) - b * b) / det
        px, py, r = pre["xy"][:, 0], pre["xy"][:, 1], torch.ceil(o["r3"])
        o["edges"] = torch.stack([(px - r) / 16, (py - r) / 16, (px + r + 15) / 16, (py + r + 15) / 16], 1)
        if cfg.sh:
            d = t(sc["means3D"]) - campos.to(dtype)[None]
            d = d / torch.sqrt((d * d).sum(1, keepdim=True))
            o["raw"] = rt.eval_sh(cfg.deg, t(sc["shs"][:, :cfg.M]), d) + 0.5
        vis = pre["valid"] & ~torch.isnan(op.reshape(-1))         # the product culls a NaN opacity (raster_pre_body.h: preprocess_geom)
        o["radii_full"] = torch.where(vis, pre["radii"], torch.zeros_like(pre["radii"])).numpy()
        if window:
            gx, gy, x0, y0 = (cfg.W + 15) // 16 + 1, (cfg.H + 15) // 16 + 1, window[2] // 16, window[3] // 16
            r0, r1, r2, r3 = pre["rect"]
            vis = vis & (torch.clamp(r2, max=x0 + gx) > torch.clamp(r0, min=x0)) & (torch.clamp(r3, max=y0 + gy) > torch.clamp(r1, min=y0))
    o = {k: v.numpy() for k, v in o.items() if torch.is_tensor(v)} | {k: v for k, v in o.items() if not torch.is_tensor(v)}
    o.update(vis=vis.numpy(), front=(pv[:, 2] > NEAR).numpy(), xy=pre["xy"].numpy(), conic=pre["conic"].numpy(),
             opacity=pre["opacity"].numpy(), clamped=(o["raw"] < 0) if cfg.sh else None)
    o["radii"] = np.where(o["vis"], o["radii_full"], 0)
    return o


def _decisions_clear(f, cfg):
    """bool (n): every threshold decision of the row is at a distance from its threshold in this float64 forward."""
    front = f["front"]
    frac = lambda x: np.abs(x - np.round(x))
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = np.abs(f["z"] - NEAR) > 1e-4
        ok &= ~front | (frac(f["r3"]) > 1e-4 * f["r3"])
        ok &= ~front | (frac(f["edges"]) > 1e-3).all(1)
        ok &= ~front | ((np.abs(np.abs(f["xz"]) / (1.3 * cfg.tanx) - 1) > 1e-3) & (np.abs(np.abs(f["yz"]) / (1.3 * cfg.tany) - 1) > 1e-3))
        if cfg.aa:
            ok &= ~front | (np.abs(f["rho"] / AA_FLOOR - 1) > 1e-2)
        if cfg.sh:
            ok &= (np.abs(f["raw"]) > 1e-3).all(1)
    return ok


def _is_kind(kind, f, cfg, nan_op):
    """bool (n): the float64 forward of view 0 puts the row in `kind`."""
    vis, gx, gy = f["vis"], np.abs(f["xz"]) > 1.3 * cfg.tanx, np.abs(f["yz"]) > 1.3 * cfg.tany
    on = vis & ~gx & ~gy
    cl = f["clamped"] if cfg.sh else np.zeros((len(vis), 3), bool)
    rule = {
        "plain_axis": on & (np.abs(f["xz"]) < 1e-6) & (np.abs(f["yz"]) < 1e-6), "plain_off": on & (np.abs(f["xz"]) > 1e-3), "plain_aniso": on,
        "guard_x": vis & gx & ~gy, "guard_y": vis & ~gx & gy, "guard_xy": vis & gx & gy,
        "tiny_below": on & (f["rho"] < AA_FLOOR), "tiny_above": on & (f["rho"] > AA_FLOOR) & (f["rho"] < 2 * AA_FLOOR),
        "huge": vis & (f["r3"] > max(cfg.Wr, cfg.Hr)),
        "near_in": vis & (f["z"] < NEAR + 2e-3), "near_out": ~vis & (f["z"] > NEAR - 2e-3) & (f["z"] < NEAR),
        "behind": ~vis & (f["z"] < 0), "offscreen": ~vis & f["front"] & ~nan_op, "nan_opacity": ~vis & f["front"] & nan_op,
        "clamp_0": on & cl[:, 0] & ~cl[:, 1] & ~cl[:, 2], "clamp_12": on & ~cl[:, 0] & cl[:, 1] & cl[:, 2], "clamp_012": on & cl.all(1),
        "rot_05": on, "rot_10": on, "rot_17": on,
    }[kind]
    if not cfg.sh and kind.startswith("clamp_"):
        rule = on                                             # precomputed colours: nothing clamps; the rows stay as plain ones
    if kind not in ("nan_opacity",):
        rule = rule & ~nan_op
    return rule


def table_kinds(P):
    """The kinds of the table's rows for a scene of P Gaussians: the full table where it fits, else one kind after the other
    round-robin over the classes, so that a small scene still meets every class it has room for."""
    per_class = [[k for k, n in zip(kinds, counts) for _ in range(n)] for _, kinds, counts in CLASS_TABLE]
    for row in per_class:                                      # interleave the kinds of a class: a cut keeps all of them
        kinds = sorted(set(row), key=row.index)
        row[:] = [k for i in range(max(map(row.count, kinds))) for k in kinds if row.count(k) > i]
    out, i = [], 0
    while len(out) < min(P, TABLE_ROWS):
        for row in per_class:
            if i < len(row) and len(out) < P:
                out.append(row[i])
        i += 1
    return out


def edge_scene(P, seed, cfg, n_views=1):
    """-> dict: the float32 inputs (means3D, scales, rotations, cov6, opacities, logits, shs, rgb), `kind` / `cls` (P,) names,
    `cams` (n_views camera dicts), `cfg`.  The table's rows sit at seeded positions among the sampler's."""
    rng = np.random.default_rng(seed)
    cams = cameras(n_views, cfg)
    kinds = table_kinds(P)
    kinds = kinds + [("plain_off", "rot_10", "plain_off", "rot_10", "plain_aniso")[i % 5] for i in range(P - len(kinds))]      # the sampler's fill
    order = rng.permutation(P)
    kinds = [kinds[i] for i in order]
    chosen = [None] * P
    for attempt in range(40):
        todo = [i for i in range(P) if chosen[i] is None]
        if not todo:
            break
        parts = [_draw(kinds[i], 1, rng, cfg) for i in todo]
        sc = _assemble(parts, cfg)
        nan_op = np.isnan(sc["opacities"]).reshape(-1)
        fs = [forward64(sc, cfg, cam) for cam in cams]
        ok = np.logical_and.reduce([_decisions_clear(f, cfg) for f in fs])
        for j, i in enumerate(todo):
            if ok[j] and _is_kind(kinds[i], fs[0], cfg, nan_op)[j]:
                chosen[i] = parts[j]
    assert all(c is not None for c in chosen), [kinds[i] for i in range(P) if chosen[i] is None]
    sc = _assemble(chosen, cfg)
    sc.update(kind=np.array(kinds), cls=np.array([KIND_CLASS[k] for k in kinds]), cams=cams, cfg=cfg, P=P)
    # the two properties of the FINAL scene, in every camera
    for cam in cams:
        f = forward64(sc, cfg, cam)
        fr = f["front"]
        assert (np.abs(f["r3"][fr] - np.round(f["r3"][fr])) > 1e-4 * f["r3"][fr]).all(), "a radius within 1e-4 of an integer"
        assert (np.abs(f["z"] - NEAR) > 1e-4).all(), "a depth within 1e-4 of the near plane"
        assert _decisions_clear(f, cfg).all()
    return sc


def class_counts(sc):
    """{kind: rows} as the FLOAT64 REFERENCE of view 0 classifies the final scene (never the code under test)."""
    cfg = sc["cfg"]
    f = forward64(sc, cfg, sc["cams"][0])
    nan_op = np.isnan(sc["opacities"]).reshape(-1)
    return {k: int((_is_kind(k, f, cfg, nan_op) & (sc["kind"] == k)).sum()) for k in KIND_CLASS}


def assert_classes(sc):
    """Every kind the table placed is what the float64 reference sees, and a scene with room for the whole table holds at least 8
    rows of every class."""
    got, placed = class_counts(sc), {k: int((sc["kind"] == k).sum()) for k in KIND_CLASS}
    assert got == placed, (got, placed)
    if sc["P"] >= TABLE_ROWS:
        for cls, kinds, _ in CLASS_TABLE:
            n = sum(got[k] for k in kinds)
            assert n >= 8 and all(got[k] >= 1 for k in kinds), (cls, got)
    return got


# ----------------------------------------------------------------------------------------------------------------------------
# the accumulator and the reference gradients
# ----------------------------------------------------------------------------------------------------------------------------
def make_acc(P, seed, invdepth=True, views=1):
    """(views P, 16) float32: every slot the per-Gaussian backward reads, on EVERY row (a culled row's record must be ignored)."""
    rng = np.random.default_rng(seed)
    acc = np.zeros((views * P, ACC_STRIDE), np.float32)
    acc[:, [0, 1, 3, 4, 5, 6, 7, 8, 9]] = rng.normal(size=(views * P, 9)).astype(np.float32)
    if invdepth:
        acc[:, 10] = rng.normal(size=views * P).astype(np.float32)
    return acc


class _GuardedDenominator(torch.autograd.Function):
    """The conic, with the backward's denominator as R6 has it: upstream forms d(conic)/d(cov2D) with 1 / (det^2 + 1e-7) where the
    derivative has 1 / det^2 (oracle/raster_c/raster_oracle.c and d3ga_math.h: cov2d_bwd restate it; oracle/raster_torch leaves it to
    autograd).  The conic's incoming gradient times det^2 / (det^2 + 1e-7) is that, exactly: up to 1.2e-5 relative on a Gaussian far
    below the dilation (det = 0.09), which the bars would otherwise report on every such row."""

    @staticmethod
    def forward(ctx, conic, k):
        ctx.save_for_backward(k)
        return conic.clone()

    @staticmethod
    def backward(ctx, g):
        (k,) = ctx.saved_tensors
        return g * k[:, None], None


def reference(sc, cfg, acc, dtype, view=0, jitter=None):
    """Gradients of the linear functional `acc` (P, 16) stands for, through oracle/raster_torch.preprocess evaluated in `dtype` in
    camera `view`, summed over the rows the FLOAT64 forward calls visible -> dict of float64 numpy arrays: means3D, opacities,
    sh | colors, cov3D | scales + rotations, and the forward's vis, radii, clamped (P, 3).
    jitter = seed: every float input moved by up to one relative float32 rounding (6e-8) first -- see references32."""
    cam = sc["cams"][view]
    f64 = forward64(sc, cfg, cam)
    idx = torch.from_numpy(np.nonzero(f64["vis"])[0])
    view_m, proj, campos = (torch.from_numpy(a) for a in cam_arrays(cam))
    jr = None if jitter is None else np.random.default_rng(jitter)

    def leaf(a):
        a = np.ascontiguousarray(a)
        if jr is not None:
            a = (a.astype(np.float64) * (1.0 + 6e-8 * jr.uniform(-1.0, 1.0, size=a.shape))).astype(np.float32)
        return torch.from_numpy(a).to(dtype).requires_grad_(True)
    m = leaf(sc["means3D"])
    g = {}
    if cfg.from_sr:
        g["scales"], g["rotations"] = leaf(sc["scales"]), leaf(sc["rotations"])
        kw = dict(scales=g["scales"], rotations=g["rotations"], scale_modifier=cfg.mod)
    else:
        g["cov3D"] = leaf(sc["cov6"])
        kw = dict(cov3D_precomp=g["cov3D"])
    if cfg.sh:
        g["sh"] = leaf(sc["shs"][:, :cfg.M])
        kw.update(shs=g["sh"], sh_degree=cfg.deg)
    else:
        g["colors"] = leaf(sc["rgb"])
        kw.update(colors_precomp=g["colors"])
    g["opacities"] = leaf(sc["logits"] if cfg.sigmoid else sc["opacities"])
    op = torch.sigmoid(g["opacities"]) if cfg.sigmoid else g["opacities"]
    Wr, Hr = cfg.Wr, cfg.Hr
    pre = rt.preprocess(m, op, view_m, proj, campos, cfg.tanx, cfg.tany, Wr, Hr, antialiasing=cfg.aa, **kw)
    a = torch.from_numpy(acc).to(dtype)[idx]
    det2 = torch.from_numpy(f64["det"] ** 2).to(dtype)
    xy, cn = pre["xy"][idx], _GuardedDenominator.apply(pre["conic"], det2 / (det2 + 0.0000001))[idx]
    # mean2D gradient in NDC-scaled units: d(pixel)/d(ndc) = W / 2
    L = (xy[:, 0] * a[:, 0] / (0.5 * Wr)).sum() + (xy[:, 1] * a[:, 1] / (0.5 * Hr)).sum()
    L = L + (cn[:, 0] * a[:, 3]).sum() + (cn[:, 1] * 2.0 * a[:, 4]).sum() + (cn[:, 2] * a[:, 5]).sum()
    L = L + (pre["rgb"][idx] * a[:, 7:10]).sum() + (pre["opacity"][idx] * a[:, 6]).sum() + (a[:, 10] / pre["depth"][idx]).sum()
    L.backward()
    g["means3D"] = m
    out = {k: (torch.zeros_like(v) if v.grad is None else v.grad).double().numpy().reshape(len(m), -1) for k, v in g.items()}
    out.update(vis=f64["vis"], radii=f64["radii"], radii_full=f64["radii_full"], clamped=f64["clamped"])
    return out


GRAD_KEYS = ("means3D", "opacities", "sh", "colors", "cov3D", "scales", "rotations")
WORST = {}                               # (first word of the tag, output, class) -> worst ratio seen by check_grads in this process


def worst_table(where):
    """The worst ratios check_grads saw under tags that start with `where`, per output and class, as text (docs/LOG.md)."""
    cls = list(dict.fromkeys(c for w, _, c in WORST if w == where))
    rows = [f"  {'':9s} " + " ".join(f"{c:>8s}" for c in cls)]
    for k in GRAD_KEYS:
        if any((where, k, c) in WORST for c in cls):
            rows.append(f"  {k:9s} " + " ".join(f"{WORST[(where, k, c)]:8.2f}" if (where, k, c) in WORST else f"{'-':>8s}" for c in cls))
    return "\n".join(rows)


def sum_views(refs):
    """The float64 sum of per-view references (shared geometry and appearance); vis = visible in some view."""
    out = {k: sum(r[k] for r in refs) for k in GRAD_KEYS if k in refs[0]}
    out["vis"] = np.logical_or.reduce([r["vis"] for r in refs])
    return out


def row_err(d, g):
    """Per row: max_j |d - g|, max_j |g|."""
    return np.abs(d - g).max(1), np.abs(g).max(1)


MIN_GROUP = 4                            # visible rows a class needs for an e32 of its own


def groups(sc):
    """(P,) group names: the classes, with the strongly anisotropic rows (scale ratios up to 1e3, whose float32 error is two orders
    above everything else's) apart from the other plain ones."""
    return np.where(sc["kind"] == "plain_aniso", "aniso", sc["cls"])


N_JITTER = 4


def references32(sc, cfg, acc, view=0):
    """The float32 evaluations e32 is taken over: the reference at the inputs, and at N_JITTER copies of them with every float moved
    by up to one relative float32 rounding (the protocol of cage_ref.reference).  One evaluation is ONE sample of a row's rounding
    error.  Where a single cancellation makes up that error -- the strongly anisotropic rows -- two samples differ by more than the
    margin of 4 about one time in seven (the ratio of two centred normal values): with one evaluation, row 81 of the host case
    sh9_deg2_cov6 stood at 9.1e-5 in the g++ build against 1.3e-5 in the float32 reference, with rows at 1e-7 .. 1e-3 around it."""
    return [reference(sc, cfg, acc, torch.float32, view)] + [reference(sc, cfg, acc, torch.float32, view, jitter=1000 + j) for j in range(N_JITTER)]


def bars(ref64, refs32, sc):
    """{output: {"all": e32, class: e32 ...}}.  e32 ("all") = the worst row error of the float32 evaluations of the reference
    (references32) against the float64 one over the visible rows, relative to the row's largest element, floored at 2^-22.  A class
    with at least MIN_GROUP visible rows has the same number over ITS rows: the rule applied to the scene that holds only that class
    (rows do not interact), so that the ill-conditioned rows of one class do not widen the bar of every other; a smaller class keeps
    "all"."""
    vis, grp, e = ref64["vis"], groups(sc), {}
    for k in GRAD_KEYS:
        if k in ref64:
            top = np.abs(ref64[k]).max(1)
            err = np.max([row_err(r[k], ref64[k])[0] for r in refs32], 0)
            rel = np.where(top > 0, err / np.where(top > 0, top, 1.0), 0.0)
            e[k] = {"all": max(E32_FLOOR, float(rel[vis].max(initial=0.0)))}
            for c in dict.fromkeys(grp):
                rows = vis & (grp == c)
                e[k][c] = max(E32_FLOOR, float(rel[rows].max())) if rows.sum() >= MIN_GROUP else e[k]["all"]
    return e


def check_grads(got, ref64, e32, sc, cfg, acc, tag, m2=None, opacity_exact=True):
    """`got` {output: (P, .) array} under the bars, and the exact properties.  Prints the worst ratio (x e32) per output and per
    class before anything is asserted -> {output: worst ratio}.  m2: dL_dmeans2D (P, 3) of the view `acc` belongs to;
    opacity_exact=False: a sum over views, where dL_dopacity is no single record's slot."""
    vis, P, grp = ref64["vis"], len(ref64["vis"]), groups(sc)
    worst, lines, fails = {}, [], []
    for k in GRAD_KEYS:
        if k not in got or got[k] is None:
            continue
        d, g = np.asarray(got[k], np.float64).reshape(P, -1), ref64[k]
        if not np.isfinite(d).all():
            fails.append(f"{k}: non-finite values")
            continue
        err, top = row_err(d, g)
        e_row = np.array([e32[k][c] for c in grp])
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(top > 0, err / (e_row * top), np.where(err > 0, np.inf, 0.0))          # against the row's class
            ratio_all = np.where(top > 0, err / (e32[k]["all"] * top), ratio)                       # against the whole scene's e32
        ratio, ratio_all = np.where(vis, ratio, 0.0), np.where(vis, ratio_all, 0.0)
        i = int(np.argmax(ratio))
        worst[k] = float(ratio[i])
        per = " ".join(f"{c} x{ratio[grp == c].max():.2f} ({e32[k][c]:.1e})" for c in dict.fromkeys(grp) if (vis & (grp == c)).any())
        for c in dict.fromkeys(grp):
            if (vis & (grp == c)).any():
                key = (tag.split()[0], k, str(c))
                WORST[key] = max(WORST.get(key, 0.0), float(ratio[grp == c].max()))
        lines.append(f"  {k:9s} worst x{worst[k]:.2f} of its class's e32 (row {i}: {sc['kind'][i]}), x{ratio_all.max():.2f} of the scene's "
                     f"{e32[k]['all']:.2e} | {per}")
        if worst[k] > MARGIN:
            fails.append(f"{k}: row {i} ({sc['kind'][i]}) x{worst[k]:.2f} of e32 = {e_row[i]:.2e} (bar x{MARGIN:g})")
        if np.abs(d[~vis]).max(initial=0.0) != 0.0:
            fails.append(f"{k}: a culled row is not zero")
    print(f"[preprocess-alone] {tag}: {cfg}, {int(vis.sum())}/{P} visible\n" + "\n".join(lines))
    if cfg.sh and got.get("sh") is not None:
        d = np.asarray(got["sh"]).reshape(P, cfg.M, 3)
        nb = (cfg.deg + 1) ** 2
        if np.abs(d[:, nb:]).max(initial=0.0) != 0.0:
            fails.append("sh: a coefficient above the active degree is not zero")
        cl = ref64.get("clamped")
        if cl is not None and np.abs(d.transpose(0, 2, 1)[cl & vis[:, None]]).max(initial=0.0) != 0.0:
            fails.append("sh: a clamped channel is not zero")
    if m2 is not None:
        m2 = np.asarray(m2).reshape(P, 3)
        if not (np.array_equal(m2[vis, :2], acc[vis, :2]) and np.all(m2[~vis] == 0) and np.all(m2[:, 2] == 0)):
            fails.append("dL_dmeans2D is not acc[:, :2] | 0 on the visible rows and zero elsewhere")
    if got.get("opacities") is not None and not cfg.aa and not cfg.sigmoid and opacity_exact:
        if not np.array_equal(np.asarray(got["opacities"]).reshape(-1)[vis], acc[vis, 6]):
            fails.append("dL_dopacity is not acc[:, 6] bit for bit")
    assert not fails, (tag, fails)
    return worst
