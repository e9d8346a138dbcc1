"""Every launch path of the compositing kernels (d3ga_amd/csrc/raster_composite.hip: forward, raster_composite_scan.hip: backward),
called through d3ga_amd._lib.lib() with raw pointers, against the C oracle (tests/composite_ref.py holds the scenes, the oracle
side and the path tables; tests/test_composite_paths_host.py checks the tables' cover on the CPU).
  forward rows   all 24 instantiations composite_fwd_q_kernel<DUAL, DEPTH, L1V, PVB, WIN> under composite_variant 0 / 32 / 128 /
                 160, forward_only, target / target_cell: colour, the pair's second image, inverse depth and the fused L1 value
                 against the oracle per view; colour, n_contrib and final_T bit for bit the plain default-knob render's; a
                 forward_only call writes nothing behind n_contrib
  backward rows  all 24 instantiations composite_bwd_tile_kernel<DUAL, S, INVD, 1, PVB, WIN> under merge_slots, tile_assign,
                 bwd_split, composite_variant and every form of the incoming gradient (dL_dpix, the fused L1 source with and
                 without it, dL_dinvdepth with and without it), each followed by d3ga_raster_preprocess_bwd: dL/dmeans3D, dL/dcov3D,
                 dL/dopacity, dL/dcolour against the oracle's backward, the incoming gradients zeroed on the oracle's marginal
                 pixels on both sides.  The `deep` scene (four tiles of > 1000 entries of which up to 631 blend) forces records out
                 of the merge cache before the tile is done, at 512 and at 256 slots.
  refusals       the status of every refused call, and nothing written.
Per camera set d3ga_raster_preprocess and d3ga_raster_bin_sort run once; every row composites on that scratch.  Every output
(out_color, out_color2, out_invdepth, loss, partials, the img buffer, acc, the gradients) sits in a guard band (cage_ref), checked
after every call.
Bars (the ones util.Parity holds the operator to): images 1e-4 on non-marginal pixels, 8e-3 on marginal ones (inverse depth
2e-2); gradients |a - b| <= 1e-3 |b| + 1e-6 max|b| on every Gaussian, plus util.conditioning_noise on the `deep` scene, whose
per-Gaussian sums have hundreds of terms; the L1 value 2e-6 relative (test_fused_l1_value_on_ragged_sizes_and_unaligned_targets).
A knob changes the backward's summation order only: each row's verdict is its distance to the oracle; its distance to the same call
under the default knobs is printed (docs/LOG.md has the table), not asserted."""
import contextlib
import ctypes
import functools

import numpy as np
import pytest
import torch

import cage_ref as cr
import composite_ref as ref
from d3ga_amd import _lib, cameras
from d3ga_amd._lib import RasterParams
from oracle import raster_c as rc
from test_gpu_mlp_paths import Frozen, knob, vp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OK, E_NULL, E_SIZE, E_CONFIG = 0, -1, -2, -3     # D3GA_* (include/d3ga.h)
ACC_STRIDE = 16                                  # D3GA_ACC_STRIDE
FWD_ROWS, BWD_ROWS = ref.fwd_table(), ref.bwd_table()


def L():
    return _lib.lib()


def S():
    return _lib.stream_handle()


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype).contiguous()


def a256(n):
    return (n + 255) // 256 * 256


@contextlib.contextmanager
def knobs(row):
    """The four compositing knobs of a row (None: the library as it is)."""
    with contextlib.ExitStack() as st:
        if row is not None:
            for name, key in (("composite_variant", "variant"), ("merge_slots", "slots"), ("tile_assign", "assign"), ("bwd_split", "split")):
                if key in row:
                    st.enter_context(knob(name, row[key]))
        yield


class DevSet:
    """A camera set on the device: the Gaussians, the cameras, and the scratch that d3ga_raster_preprocess + d3ga_raster_bin_sort
    filled once (checked against the oracle: radii, and without a window the duplicate count)."""

    def __init__(self, name):
        scene, k, win = ref.SETS[name]
        vs, g = ref.views(name), ref.gaussians(scene)
        self.name, self.scene, self.k, self.win, self.P, self.W, self.H = name, scene, k, win, g["means3D"].shape[0], vs[0].W, vs[0].H
        self.means, self.cov6, self.opac, self.rgb, self.colors2 = (g[x].to(DEV) for x in ("means3D", "cov6", "opacities", "rgb", "colors2"))
        if win:
            rows = [cameras.window_row_host(v.batch) for v in vs]
            self.view, self.proj = dev(np.stack([r[0:16] for r in rows])), dev(np.stack([r[32:48] for r in rows]))
            self.campos, tan = dev(np.stack([r[48:57] for r in rows])), (cameras.CAMERA_SLOT_WINDOWED,) * 2
        else:
            self.view, self.proj = dev(np.stack([v.view for v in vs])), dev(np.stack([v.proj for v in vs]))
            self.campos, tan = dev(np.stack([v.campos for v in vs])), (vs[0].cam["tanfovx"], vs[0].cam["tanfovy"])
        self.prm = RasterParams(P=self.P, M=0, sh_degree=0, W=self.W, H=self.H, tanfovx=tan[0], tanfovy=tan[1], scale_modifier=1.0,
                                n_views=k if k > 1 else 0)
        self.cap = 16384 * k
        self.tiles = ((self.W + 15) // 16 + win) * ((self.H + 15) // 16 + win) * k
        self.sizes = {fo: self._sizes(fo) for fo in (0, 1)}
        if not win and k == 1:
            assert self.sizes[1][2] == L().d3ga_raster_img_bytes(self.W, self.H, self.cap, 1) == 2 * a256(4 * self.W * self.H)
            assert self.sizes[0][2] == L().d3ga_raster_img_bytes(self.W, self.H, self.cap, 0)
        self.geom = torch.zeros(self.sizes[0][0], dtype=torch.uint8, device=DEV)
        self.binning = torch.zeros(self.sizes[0][1], dtype=torch.uint8, device=DEV)
        self.radii = torch.zeros(k * self.P, dtype=torch.int32, device=DEV)
        p = ctypes.byref(self.prm)
        assert L().d3ga_raster_preprocess(p, vp(self.means), None, vp(self.rgb), vp(self.opac), None, None, vp(self.cov6), vp(self.view),
                                          vp(self.proj), vp(self.campos), vp(self.geom), vp(self.binning), self.cap, vp(self.radii), S()) == OK
        assert L().d3ga_raster_bin_sort(p, vp(self.geom), vp(self.binning), self.cap, S()) == OK
        torch.cuda.synchronize()
        cnt = self.binning[:32].view(torch.int32).cpu().tolist()
        assert cnt[1] == 0, "tile lists truncated"
        renders = [ref.render(name, v) for v in range(k)]
        assert np.array_equal(self.radii.cpu().numpy().reshape(k, self.P), np.stack([r.radii for r in renders]))
        if not win:
            assert cnt[0] == sum(rc.num_rendered(r.ctx) for r in renders)
        self._plain = {}

    def _sizes(self, forward_only):
        s = (ctypes.c_int64 * 3)()
        fn = L().d3ga_raster_scratch_bytes_window if self.win else L().d3ga_raster_scratch_bytes_views
        assert fn(self.P, self.W, self.H, self.k, self.cap, forward_only, s) == OK
        return tuple(int(x) for x in s)

    def prm_of(self, pvb=False, forward_only=False, **fields):
        p = RasterParams.from_buffer_copy(self.prm)
        p.per_view_background, p.forward_only = int(pvb), int(forward_only)
        for f, v in fields.items():
            setattr(p, f, v)
        return p

    def bg(self, pvb):
        return dev(np.asarray([ref.background(pvb, v) for v in range(self.k)] if pvb else ref.BG0, np.float32))

    def plain(self, pvb):
        """The plain render of this set under the library's own knobs: what every row's colour, n_contrib and final_T must equal
        bit for bit."""
        if pvb not in self._plain:
            self._plain[pvb] = run_forward(self, "plain", False, pvb, False)
        return self._plain[pvb]


@functools.lru_cache(maxsize=None)
def dev_set(name):
    return DevSet(name)


def device_cell(t):
    """A device cell holding the address of `t` (graph.TensorSlot's form of a target)."""
    return torch.tensor([t.data_ptr()], dtype=torch.int64, device=DEV)


class Fwd:
    pass


def run_forward(ds, mode, depth, pvb, forward_only, target_form="target", row=None):
    """One compositing forward of `mode` into guarded outputs under the knobs of `row` -> the outputs, every guard checked."""
    k, H, W = ds.k, ds.H, ds.W
    prm = ds.prm_of(pvb, forward_only)
    o = Fwd()
    o.prm, o.bg, o.bg2 = prm, ds.bg(pvb), dev(np.asarray(ref.BG2, np.float32))
    o.img = cr.GuardedWords("img", (ds.sizes[int(forward_only)][2] // 4,), DEV)
    o.color = cr.GuardedBuffer("out_color", (k, 3, H, W), DEV)
    o.color2 = cr.GuardedBuffer("out_color2", (k, 3, H, W), DEV) if mode == "pair" else None
    o.invd = cr.GuardedBuffer("out_invdepth", (k, H, W), DEV) if depth else None
    o.loss = o.partials = None
    p, com = ctypes.byref(prm), (vp(ds.geom), vp(ds.binning), ds.cap, vp(o.img), vp(o.color))
    with knobs(row):
        if mode == "pair":
            st = L().d3ga_raster_composite_fwd2(p, vp(o.bg), vp(o.bg2), vp(ds.geom), vp(ds.colors2), vp(ds.binning), ds.cap, vp(o.img),
                                                vp(o.color), vp(o.color2), vp(o.invd), S())
        elif mode == "l1":
            o.loss, o.partials = cr.GuardedBuffer("loss", (1,), DEV), cr.GuardedBuffer("partials", (4 * ds.tiles,), DEV)
            o.target = dev(ref.incoming(ds.name, pvb)["target"])
            o.cell = device_cell(o.target)
            tgt, cell = (o.target, None) if target_form == "target" else (None, o.cell)
            st = L().d3ga_raster_composite_fwd_l1(p, vp(o.bg), *com, vp(o.invd), vp(tgt), vp(cell), vp(o.loss), vp(o.partials), S())
        else:
            st = L().d3ga_raster_composite_fwd(p, vp(o.bg), *com, vp(o.invd), S())
    assert st == OK, st
    torch.cuda.synchronize()
    for b in (o.color, o.color2, o.invd, o.loss, o.partials):
        if b is not None:
            b.check()
    o.img.check(first=0)                             # the bands: forward_only -> nothing behind n_contrib's section
    n = k * H * W
    o.final_T = o.img.t[:n].view(torch.float32)
    o.n_contrib = o.img.t[a256(4 * n) // 4:a256(4 * n) // 4 + n]
    assert not bool((o.n_contrib == cr.FILL).any()) and not bool(torch.isnan(o.final_T).any()), "final_T / n_contrib not written everywhere"
    return o


def assert_image(par, got, want, tag, marginal_atol=8e-3):
    ok, strict, loose, n = par.image(got, want, marginal_atol=marginal_atol)
    print(f"[composite-paths] {tag}: non-marginal {strict:.3e} (bar 1e-4), {n} marginal pixels {loose:.3e} (bar {marginal_atol:g})")
    assert ok, (tag, strict, loose, n)


@pytest.mark.parametrize("row", FWD_ROWS, ids=[r["id"] for r in FWD_ROWS])
def test_forward_row(row):
    ds = dev_set(row["set"])
    base = ds.plain(row["pvb"])
    o = run_forward(ds, row["mode"], row["depth"], row["pvb"], row["forward_only"], row["target"], row)
    assert torch.equal(o.color.t, base.color.t), f"colour differs from the plain default-knob render: {float((o.color.t - base.color.t).abs().max()):.3e}"
    assert torch.equal(o.n_contrib, base.n_contrib) and torch.equal(o.final_T, base.final_T), "n_contrib / final_T differ from the plain render's"
    color = o.color.t.cpu().numpy()
    renders = ref.row_renders(row["set"], row["pvb"])
    for v, r in enumerate(renders):
        assert_image(r.par, color[v], r.color, f"{row['id']} view {v} colour")
        if row["depth"]:
            assert_image(r.par, o.invd.t[v].cpu().numpy(), r.invd, f"{row['id']} view {v} inverse depth", marginal_atol=2e-2)
    if row["mode"] == "pair":
        c2 = o.color2.t.cpu().numpy()
        for v, r2 in enumerate(ref.row_renders(row["set"], row["pvb"], second=True)):
            assert_image(r2.par, c2[v], r2.color, f"{row['id']} view {v} second image")
    if row["mode"] == "l1":
        tgt = ref.incoming(row["set"], row["pvb"])["target"].astype(np.float64)
        want = float(np.abs(np.stack([r.color for r in renders]).astype(np.float64) - tgt).mean())
        own = float(np.abs(color.astype(np.float64) - tgt).mean())
        loss = float(o.loss.t[0])
        print(f"[composite-paths] {row['id']} L1 value {loss:.9g}: oracle image {want:.9g} (rel {abs(loss - want) / want:.2e}), "
              f"the device's own image {own:.9g} (rel {abs(loss - own) / own:.2e}); bar 2e-6")
        assert abs(loss - want) <= 2e-6 * want, (loss, want)


# ----------------------------------------------------------------------------------------------------------------------------
# backward
# ----------------------------------------------------------------------------------------------------------------------------
def run_backward(ds, mode, src, pvb, row=None):
    """The forward that leaves the per-block lists, one compositing backward of (mode, src) and d3ga_raster_preprocess_bwd, all
    under the knobs of `row` -> {means3D, cov3D, opacities, colors} numpy float64 (P, .), every guard checked."""
    k, P, H, W = ds.k, ds.P, ds.H, ds.W
    inc = ref.incoming(ds.name, pvb)
    with knobs(row):
        f = run_forward(ds, "pair" if mode == "pair" else "plain", False, pvb, False)      # (no knob() of its own: the block's hold)
        acc = cr.GuardedBuffer("acc", (k * P, ACC_STRIDE), DEV)
        acc.t.zero_()
        gpix = dev(inc["gpix"]) if "dpix" in src else None
        p, com = ctypes.byref(f.prm), (vp(ds.geom), vp(ds.binning), ds.cap, vp(f.img))
        fz = Frozen(f.img, f.color, f.color2)
        if mode == "pair":
            st = L().d3ga_raster_composite_bwd2(p, vp(f.bg), vp(f.bg2), vp(ds.geom), vp(ds.colors2), vp(ds.binning), ds.cap, vp(f.img),
                                                vp(gpix), vp(dev(inc["gpix2"])), vp(acc), S())
        elif mode == "depth":
            st = L().d3ga_raster_composite_bwd_depth(p, vp(f.bg), *com, vp(gpix), vp(dev(inc["gd"])), vp(acc), S())
        elif src.startswith("l1"):
            target = dev(inc["target"])
            image = f.color.t.clone()                 # the forward's colour; on the marginal pixels := the target, so that the
            m = dev(inc["pix"], torch.bool)[:, None].expand(k, 3, H, W)      # L1 term is zero there (the masked protocol)
            image[m] = target[m]
            cell = device_cell(target)
            tgt, cl = (target, None) if src.startswith("l1t") else (None, cell)
            st = L().d3ga_raster_composite_bwd_l1(p, vp(f.bg), *com, vp(image), vp(tgt), vp(cl), vp(dev(inc["g_loss"].reshape(1))),
                                                  vp(gpix), vp(acc), S())
        else:
            st = L().d3ga_raster_composite_bwd(p, vp(f.bg), *com, vp(gpix), vp(acc), S())
        assert st == OK, st
        torch.cuda.synchronize()
    acc.check()
    fz.same("compositing backward (its inputs)")
    g = dict(means3D=cr.GuardedBuffer("dL_dmeans3D", (P, 3), DEV), means2D=cr.GuardedBuffer("dL_dmeans2D", (k, P, 3), DEV),
             opacities=cr.GuardedBuffer("dL_dopacity", (P, 1), DEV), colors=cr.GuardedBuffer("dL_dcolors", (P, 3), DEV),
             cov3D=cr.GuardedBuffer("dL_dcov3D", (P, 6), DEV))
    st = L().d3ga_raster_preprocess_bwd(p, vp(ds.means), None, None, None, vp(ds.cov6), vp(ds.view), vp(ds.proj), vp(ds.campos), vp(ds.geom),
                                        vp(acc), vp(g["means3D"]), vp(g["means2D"]), vp(g["opacities"]), None, vp(g["colors"]), vp(g["cov3D"]),
                                        None, None, S())
    assert st == OK, st
    torch.cuda.synchronize()
    for b in g.values():
        b.check()
    acc.check()
    return {key: g[key].t.cpu().double().numpy().reshape(P, -1) for key in ref.GRAD_KEYS}


@pytest.mark.parametrize("row", BWD_ROWS, ids=[r["id"] for r in BWD_ROWS])
def test_backward_row(row):
    """One row of the backward table against the oracle's backward (see the module's docstring for the protocol and the bar).
    The `deep` rows are the regression test of the block moments' rounding: while composite_bwd_tile_kernel centred the second
    moments of a 4 x 4 block from sums about the block's origin, rows 00, 02 and 03 failed on dL/dcov3D (x1.03, x1.93, x1.93: the
    yy entry of two Gaussians half a pixel thin in y, whose dL/dconic.c carried the absolute error of a dL/dconic.a 100 x its
    size); with the moments centred as they are summed the nine rows stand at x0.06 to x0.21 (docs/LOG.md, "Compositing: every
    launch path under test")."""
    ds = dev_set(row["set"])
    deep = row["scene"] == "deep"
    want, noise = ref.oracle_gradients(row["set"], row["pvb"], row["mode"], row["src"], deep)
    # (the inverse depth alone carries no colour gradient: the oracle's is exactly zero, and so must the device's be)
    assert all(np.abs(want[key]).max() > 0 for key in ref.GRAD_KEYS if (key, row["src"]) != ("colors", "invd"))
    got = run_backward(ds, row["mode"], row["src"], row["pvb"], row)
    worst = {key: ref.grad_excess(got[key], want[key], None if noise is None else noise[key]) for key in ref.GRAD_KEYS}
    line = f"[composite-paths] {row['id']} oracle excess " + " ".join(f"{key} x{val:.3f}" for key, val in worst.items())
    if not ref.is_default_knobs(row):                 # informational: the same call under the library's own knobs
        base = run_backward(ds, row["mode"], row["src"], row["pvb"])
        line += " | to default knobs " + " ".join(
            f"{key} {np.abs(got[key] - base[key]).max() / max(np.abs(base[key]).max(), 1e-300):.2e}" for key in ref.GRAD_KEYS)
    print(line)
    assert max(worst.values()) <= 1.0, worst


def test_deep_scene_fills_the_merge_cache_on_the_device():
    """The device's own lists of the `deep` scene are the oracle's (1318, 1167, 1182, 1042 entries), and the per-block lists the
    forward wrote hold more than 512 distinct positions in some tile: records must leave a 512-slot cache before the tile is done."""
    ds = dev_set("deep1")
    off = (ctypes.c_int64 * 6)()
    assert L().d3ga_raster_binning_layout(ds.W, ds.H, ds.cap, off) == OK
    start = ds.binning[off[2]:off[2] + 4 * 5].view(torch.int32).cpu().numpy()
    ostart, _ = rc.tile_lists(ref.render("deep1", 0).ctx)
    assert np.array_equal(start, ostart)
    f = ds.plain(False)
    o2 = (ctypes.c_int64 * 2)()
    assert L().d3ga_raster_img_layout_blocks(ds.W, ds.H, o2) == OK
    words = f.img.t
    counts = words[o2[0] // 4:o2[0] // 4 + 16 * 4].cpu().numpy().reshape(4, 16)
    lists = words[o2[1] // 4:o2[1] // 4 + 2 * 16 * int(start[-1])].cpu().numpy().reshape(-1, 2)
    distinct = []
    for t in range(4):
        n, seen = int(start[t + 1] - start[t]), set()
        for b in range(16):
            at = 16 * int(start[t]) + b * n
            seen |= set(lists[at:at + counts[t, b], 0].tolist())
        distinct.append(len(seen))
    print(f"[composite-paths] deep scene: positions walked per tile {distinct}, the oracle's blending entries {ref.deep_facts()['alive']}")
    assert max(distinct) >= 512 + 64, distinct


# ----------------------------------------------------------------------------------------------------------------------------
# refusals: the status, and nothing written
# ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    """Every refusal of d3ga_raster_composite_fwd / _fwd_l1 / _fwd2 / _bwd / _bwd_depth / _bwd2 / _bwd_l1 and, through them, of
    d3ga_raster_backward / _backward_l1: the status, every guarded output as it was, acc still zero.  (colors2 together with the
    L1 partials, D3GA_E_CONFIG inside composite_fwd_impl, cannot be asked for through the exported entry points: _fwd_l1 has no
    colors2 and _fwd2 no partials; composite_ref.fwd_instance mirrors it and the host test holds it.)"""
    ds = dev_set("small1")
    k, P, H, W = ds.k, ds.P, ds.H, ds.W
    f = run_forward(ds, "pair", True, False, False)                      # a valid img buffer with its per-block lists
    fl = run_forward(ds, "l1", False, False, False)
    inc = ref.incoming("small1", False)
    gpix, gpix2, gd, target = dev(inc["gpix"]), dev(inc["gpix2"]), dev(inc["gd"]), dev(inc["target"])
    g_loss, cell = dev(inc["g_loss"].reshape(1)), device_cell(dev(inc["target"]))
    acc = cr.GuardedBuffer("acc", (k * P, ACC_STRIDE), DEV)
    acc.t.zero_()
    grads = [cr.GuardedBuffer(n, s, DEV) for n, s in (("dL_dmeans3D", (P, 3)), ("dL_dmeans2D", (P, 3)), ("dL_dopacity", (P, 1)),
                                                      ("dL_dcolors", (P, 3)), ("dL_dcov3D", (P, 6)))]
    fz = Frozen(f.img, f.color, f.color2, f.invd, fl.loss, fl.partials, acc, *grads)
    prm, fo, p0 = ds.prm_of(), ds.prm_of(forward_only=True), ds.prm_of(P=0)
    neg = ds.prm_of(W=0)
    A = dict(prm=prm, bg=f.bg, bg2=f.bg2, geom=ds.geom, binning=ds.binning, cap=ds.cap, img=f.img, color=f.color, color2=f.color2,
             invd=f.invd, colors2=ds.colors2, target=target, cell=None, loss=fl.loss, partials=fl.partials, gpix=gpix, gpix2=gpix2, gd=gd,
             image=f.color, g_loss=g_loss, acc=acc)

    def call(name, **kw):
        a = dict(A, **kw)
        p = None if a["prm"] is None else ctypes.byref(a["prm"])
        v = lambda key: vp(a[key])
        com = (v("geom"), v("binning"), a["cap"], v("img"))
        if name == "fwd":
            return L().d3ga_raster_composite_fwd(p, v("bg"), *com, v("color"), v("invd"), S())
        if name == "fwd_l1":
            return L().d3ga_raster_composite_fwd_l1(p, v("bg"), *com, v("color"), v("invd"), v("target"), v("cell"), v("loss"), v("partials"), S())
        if name == "fwd2":
            return L().d3ga_raster_composite_fwd2(p, v("bg"), v("bg2"), v("geom"), v("colors2"), v("binning"), a["cap"], v("img"), v("color"),
                                                  v("color2"), v("invd"), S())
        if name == "bwd":
            return L().d3ga_raster_composite_bwd(p, v("bg"), *com, v("gpix"), v("acc"), S())
        if name == "bwd_depth":
            return L().d3ga_raster_composite_bwd_depth(p, v("bg"), *com, v("gpix"), v("gd"), v("acc"), S())
        if name == "bwd2":
            return L().d3ga_raster_composite_bwd2(p, v("bg"), v("bg2"), v("geom"), v("colors2"), v("binning"), a["cap"], v("img"), v("gpix"),
                                                  v("gpix2"), v("acc"), S())
        if name == "bwd_l1":
            return L().d3ga_raster_composite_bwd_l1(p, v("bg"), *com, v("image"), v("target"), v("cell"), v("g_loss"), v("gpix"), v("acc"), S())
        pre = (p, vp(ds.means), None, None, None, vp(ds.cov6), vp(ds.view), vp(ds.proj), vp(ds.campos), v("bg"), *com)
        out = (v("acc"), vp(grads[0]), vp(grads[1]), vp(grads[2]), None, vp(grads[3]), vp(grads[4]), None, None, S())
        if name == "backward":
            return L().d3ga_raster_backward(*pre, v("gpix"), *out)
        assert name == "backward_l1"
        return L().d3ga_raster_backward_l1(*pre, v("image"), v("target"), v("cell"), v("g_loss"), v("gpix"), *out)

    fwds, bwds = ("fwd", "fwd_l1", "fwd2"), ("bwd", "bwd_depth", "bwd2", "bwd_l1")
    cases = []
    for n in fwds + bwds:                                                    # every required pointer, a size, the capacity
        cases += [(n, {key: None}, E_NULL) for key in ("prm", "bg", "geom", "binning", "img")]
        cases += [(n, dict(prm=neg), E_SIZE), (n, dict(cap=-1), E_SIZE)]
    cases += [(n, dict(color=None), E_NULL) for n in fwds]
    cases += [(n, dict(acc=None), E_NULL) for n in bwds]
    cases += [("fwd_l1", dict(loss=None), E_NULL), ("fwd_l1", dict(partials=None), E_NULL), ("fwd_l1", dict(target=None, cell=None), E_NULL),
              ("fwd2", dict(colors2=None), E_NULL), ("fwd2", dict(bg2=None), E_NULL), ("fwd2", dict(color2=None), E_NULL),
              ("bwd", dict(gpix=None), E_NULL), ("bwd_depth", dict(gpix=None, gd=None), E_NULL),
              ("bwd2", dict(colors2=None), E_NULL), ("bwd2", dict(gpix=None), E_NULL), ("bwd2", dict(bg2=None), E_NULL), ("bwd2", dict(gpix2=None), E_NULL),
              ("bwd_l1", dict(image=None), E_NULL), ("bwd_l1", dict(image=None, gpix=None), E_NULL),       # all incoming gradients NULL
              ("bwd_l1", dict(target=None, cell=None), E_NULL), ("bwd_l1", dict(g_loss=None), E_NULL)]
    cases += [(n, dict(prm=fo), E_CONFIG) for n in bwds + ("backward", "backward_l1")]                    # no per-block lists to walk
    cases += [(n, dict(prm=p0), OK) for n in bwds]                          # nothing to do is not a refusal: nothing launched
    cases += [("bwd", dict(prm=p0, gpix=None), OK), ("bwd_depth", dict(prm=p0, gpix=None, gd=None), OK)]
    for name, kw, want in cases:
        tag = f"{name}({', '.join(f'{key}={None if val is None else key}' for key, val in kw.items())})"
        assert call(name, **kw) == want, tag
        fz.same(tag)
    assert float(acc.t.abs().sum()) == 0.0
    # the base call of every case above is a valid one
    for n in fwds + bwds:
        assert call(n) == OK, n
    assert call("fwd_l1", target=None, cell=cell) == OK and call("bwd_l1", target=None, cell=cell, gpix=None) == OK
    assert call("bwd_depth", gpix=None) == OK
    torch.cuda.synchronize()
    assert float(acc.t.abs().sum()) > 0.0


def test_knobs_are_back_at_their_defaults():
    """Runs last in this file: every knob() block restored what it changed."""
    d = _lib.debug_defaults()
    import os
    if not os.environ.get("D3GA_KNOBS"):
        assert all(d[name][0] == d[name][1] for name in _lib.KNOBS), d
