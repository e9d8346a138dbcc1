"""The evaluation tail on the GPU (d3ga_amd/evaluation.py, csrc/eval.hip) against the float64 oracle (tests/eval_ref.py) and
the reference's own results (tests/golden/eval_cases.npz), at the smallest shapes at which the kernels can go wrong
(eval_ref.GPU_CASES): W not a multiple of 4 and the pixel-by-pixel path, the quad path, W smaller than a wavefront, several
workgroups per frame, frames of a batch with different content.

Bars (derived in tests/test_evaluation_host.py and the issue behind this module):
  target, ground_truth   <= 1e-6 against the float64 composition (the bar compose_target takes)
  heat map               bit-identical to table[bin] on every pixel whose float64 error is exactly 0, >= 1 + 4e-7 or farther
                         than 4e-7 from a multiple of 1/256; the others (at most 0.1 % of a case) may be one bin off
  PSNR                   <= 1e-3 dB against float64;  identical images give +inf
  SSIM                   <= 2e-6 against the reference's value (the bar test_gpu_parity.py holds d3ga_ssim_fwd to)
"""
import ctypes

import numpy as np
import pytest
import torch

import eval_ref as er

pytestmark = pytest.mark.gpu
DEV = "cuda"
COMPOSE_BAR, PSNR_BAR, SSIM_BAR = 1e-6, 1e-3, 2e-6
GUARD = 64                                        # floats in front of and behind every output (keeps the 16-byte alignment)
NAN_BITS = 0x7FC0DEAD                             # a NaN pattern no kernel would produce
PAIRS = ("a", "b", "c", "wide")
OUTPUTS = ("target", "ground_truth", "heatmap", "ssim", "psnr")


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _boundary(b, kind):
    return {"uint8": b, "bool": b.astype(np.bool_), "float32": b.astype(np.float32)}[kind]


@pytest.fixture(scope="module")
def cases():
    """Inputs and float64 references of every case, computed once: (seed,B,H,W) -> dict."""
    out = {}
    for seed, B, H, W in er.GPU_CASES:
        for channels in (1, 3):
            pred, image, alpha, boundary = er.make_frame_inputs(seed, B, H, W, channels)
            ref = {bg: er.compose_ref(image, alpha, boundary, 1.0 if bg == "white" else 0.0) for bg in ("white", "black")}
            out[(B, H, W, channels)] = dict(pred=pred, image=image, alpha=alpha, boundary=boundary, ref=ref)
    return out


def _check_frames(got, c, bg):
    """One Evaluator.add result against the oracle."""
    want_t, want_g = c["ref"][bg]
    target = got["target"].cpu().numpy()
    assert float(np.abs(target - want_t).max()) <= COMPOSE_BAR
    assert float(np.abs(got["ground_truth"].cpu().numpy() - want_g).max()) <= COMPOSE_BAR
    n_open, n = er.check_heat(got["heatmap"].cpu().numpy(), target, c["pred"])      # the heat of the target the kernel composed
    want_p = er.psnr_ref(target, c["pred"])
    psnr = got["psnr"].cpu().numpy()
    print(f"{target.shape} {bg}: {n_open} of {n} pixels open, psnr off by {float(np.abs(psnr - want_p).max()):.2e} dB")
    assert float(np.abs(psnr - want_p).max()) <= PSNR_BAR
    assert float(np.abs(psnr - er.psnr_ref(want_t, c["pred"])).max()) <= PSNR_BAR


@pytest.mark.parametrize("seed,B,H,W", er.GPU_CASES)
def test_batches_against_the_oracle(cases, seed, B, H, W):
    from d3ga_amd import Evaluator
    first = {}
    for channels in (1, 3):
        c = cases[(B, H, W, channels)]
        pred, image, alpha = _dev(c["pred"], c["image"], c["alpha"])
        for bg in ("white", "black"):
            for kind in ("uint8", "bool", "float32"):
                (boundary,) = _dev(_boundary(c["boundary"], kind))
                got = Evaluator(bg).add(pred, image, alpha, boundary)
                assert got["target"].shape == (B, 3, H, W) and got["ground_truth"].shape == (B, 4, H, W)
                assert got["ssim"].shape == (B,) and got["psnr"].shape == (B,)
                _check_frames(got, c, bg)
                ref = first.setdefault((channels, bg), got)       # the three boundary dtypes: the same bits
                for k in ("target", "ground_truth", "heatmap", "psnr"):
                    assert torch.equal(got[k], ref[k]), (k, kind)
        # alpha's other channels are never read: (B,3,H,W) with channel 0 of the one-channel case gives its bits
    one, three = cases[(B, H, W, 1)], cases[(B, H, W, 3)]
    mixed = three["alpha"].copy()
    mixed[:, 0] = one["alpha"][:, 0]
    pred, image, alpha, boundary = _dev(one["pred"], one["image"], mixed, one["boundary"])
    got = Evaluator("white").add(pred, image, alpha, boundary)
    for k in ("target", "ground_truth", "heatmap", "psnr"):
        assert torch.equal(got[k], first[(1, "white")][k]), k


@pytest.mark.parametrize("seed,B,H,W", er.GPU_CASES)
def test_single_frames_equal_the_batch_bit_for_bit(cases, seed, B, H, W):
    from d3ga_amd import Evaluator
    c = cases[(B, H, W, 1)]
    pred, image, alpha, boundary = _dev(c["pred"], c["image"], c["alpha"], c["boundary"])
    batch = Evaluator("black").add(pred, image, alpha, boundary)
    for b in range(B):
        one = Evaluator("black").add(pred[b], image[b], alpha[b], boundary[b])
        assert one["target"].shape == (3, H, W) and one["ground_truth"].shape == (4, H, W) and one["ssim"].shape == ()
        for k in OUTPUTS:
            assert torch.equal(one[k], batch[k][b]), (k, b)
    if B > 1:                                                 # frames with different content: an index slip would show
        assert not torch.equal(batch["psnr"][0], batch["psnr"][1]) and not torch.equal(batch["ssim"][0], batch["ssim"][1])


def test_goldens_on_the_device(golden):
    from d3ga_amd import compute_errors, compute_heatmap, error_heatmap, psnr
    z = golden("eval_cases.npz")
    table = np.concatenate([z["table"], np.zeros((1, 3), np.uint8)])
    for name in PAIRS:
        gt, pred = z[f"{name}_gt"], z[f"{name}_pred"]
        target, fake = _dev(gt, pred)
        heat, s, p, l = compute_errors(target, fake)
        assert heat.is_cuda and heat.dtype == torch.float32 and heat.shape == gt.shape
        assert isinstance(s, float) and isinstance(p, float) and np.isnan(l)
        er.check_heat(heat.cpu().numpy(), gt, pred, table)
        er.check_heat(z[f"{name}_heat"], gt, pred, table)
        print(f"{name}: ssim {s:.7f} (reference {float(z[f'{name}_ssim']):.7f}), psnr {p:.6f} (reference {float(z[f'{name}_psnr']):.6f}), "
              f"{int((heat.cpu().numpy() != z[f'{name}_heat']).any(0).sum())} pixels differ from the reference's float32 heat map")
        assert abs(s - float(z[f"{name}_ssim"])) <= SSIM_BAR
        assert abs(p - float(z[f"{name}_psnr"])) <= PSNR_BAR and abs(p - float(er.psnr_ref(gt, pred))) <= PSNR_BAR
        heat2, p2 = compute_heatmap(target, fake)
        assert isinstance(heat2, np.ndarray) and heat2.dtype == np.float32 and heat2.shape == (gt.shape[1], gt.shape[2], 3)
        assert np.array_equal(heat2, heat.permute(1, 2, 0).cpu().numpy()) and p2 == p
        per_channel = psnr(fake, target)
        assert per_channel.shape == (3, 1) and per_channel.is_cuda
        assert float(np.abs(per_channel.cpu().numpy() - z[f"{name}_psnr_channels"]).max()) <= PSNR_BAR
        h3, s3, p3 = error_heatmap(target, fake)
        assert torch.equal(h3, heat) and s3.shape == () and float(p3) == p and abs(float(s3) - s) <= SSIM_BAR
        assert compute_errors(target, fake, lpips=lambda f, t: (f - t).abs().mean())[3] == pytest.approx(float(np.abs(gt - pred).mean()), rel=1e-5)
    # the ramp and the edge values as one-row images: the error sits in one channel
    for key in ("ramp", "edge"):
        e = z[key]
        fake = np.zeros((3, 1, len(e)), np.float32)
        fake[1, 0] = e
        heat, _, _ = error_heatmap(*_dev(np.zeros_like(fake), fake))
        got = heat.cpu().numpy()[:, 0].T
        assert np.array_equal(got, table[er.heat_bins(e)].astype(np.float32) / np.float32(255)), key
        assert np.array_equal(np.round(got * 255).astype(np.uint8), z[f"{key}_heat"]), key


def test_identical_images_and_nan():
    from d3ga_amd import compute_errors, error_heatmap
    gt, pred = er.make_pair(7, 9, 11)
    (t,) = _dev(gt)
    heat, s, p, _ = compute_errors(t, t.clone())
    lut = er.jet_table_ref().astype(np.float32) / np.float32(255)
    assert p == float("inf") and abs(s - 1.0) <= SSIM_BAR
    assert (heat.permute(1, 2, 0).cpu().numpy() == lut[0]).all()
    bad = pred.copy()
    bad[2, 4, 5] = np.nan
    heat, s, p = error_heatmap(t, _dev(bad)[0])
    h = heat.permute(1, 2, 0).cpu().numpy()
    assert (h[4, 5] == 0).all() and np.isnan(float(p))
    ok = np.ones((9, 11), bool)
    ok[4, 5] = False
    want, _, _ = er.heatmap_ref(gt, pred)
    assert np.array_equal(h[ok], np.moveaxis(want, 0, -1)[ok])


def test_raw_entry_points_stay_inside_their_buffers(cases):
    """Every output between guard bands, every output alone and all together, quads and single pixels."""
    from d3ga_amd import _lib
    L = _lib.lib()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    for (B, H, W) in ((3, 70, 131), (2, 33, 16)):
        c = cases[(B, H, W, 1)]
        pred, image, alpha, boundary = _dev(c["pred"], c["image"], c["alpha"], c["boundary"])
        npart = L.d3ga_eval_partials(H, W)
        shapes = {"target": (B, 3, H, W), "gt": (B, 4, H, W), "heat": (B, 3, H, W), "partials": (B, 3, npart)}

        def run(names):
            bufs = {}
            for k in names:
                n = int(np.prod(shapes[k]))
                raw = torch.full((n + 2 * GUARD,), NAN_BITS, dtype=torch.int32, device=DEV)
                bufs[k] = (raw, raw[GUARD:GUARD + n].view(torch.float32).view(shapes[k]))
            view = lambda k: p(bufs[k][1]) if k in bufs else None
            st = L.d3ga_eval_frames(B, H, W, 1, p(pred), p(image), p(alpha), p(boundary), view("target"), view("gt"), view("heat"),
                                    view("partials"), _lib.stream_handle())
            assert st == 0
            torch.cuda.synchronize()
            for k, (raw, v) in bufs.items():
                assert (raw[:GUARD] == NAN_BITS).all() and (raw[-GUARD:] == NAN_BITS).all(), k
                assert not (v.view(torch.int32) == NAN_BITS).any(), k          # every element written
            return {k: v for k, (raw, v) in bufs.items()}

        full = run(("target", "gt", "heat", "partials"))
        assert npart == -(-H * W // 4096)
        for k in shapes:
            assert torch.equal(run((k,))[k], full[k]), k
        # the partials are the squared error of the workgroup's 4096 pixels
        d = (full["target"].double() - pred.double()) ** 2
        want = torch.stack([d.view(B, 3, -1)[:, :, i * 4096:(i + 1) * 4096].sum(-1) for i in range(npart)], -1)
        assert float(((full["partials"].double() - want).abs() / want).max()) <= 64 * 2.0 ** -24


def _frames(cases):
    c = cases[(3, 70, 131, 1)]
    return c, _dev(c["pred"], c["image"], c["alpha"], c["boundary"])


def test_evaluator_sums_singles_and_batches_alike(cases):
    from d3ga_amd import Evaluator
    c, (pred, image, alpha, boundary) = _frames(cases)
    a, b = Evaluator("white"), Evaluator("white")
    out = a.add(pred, image, alpha, boundary)
    for i in range(3):
        b.add(pred[i], image[i], alpha[i], boundary[i])
    sa, sb = a.summary(), b.summary()
    assert sa["count"] == sb["count"] == 3 and np.isnan(sa["lpips"])
    for k in ("ssim", "psnr"):
        assert abs(sa[k] - sb[k]) <= 1e-12 * abs(sa[k]), k
        assert abs(sa[k] - float(out[k].double().mean())) <= 1e-12 * abs(sa[k]), k
    a.add(pred[:2], image[:2], alpha[:2], boundary[:2])
    assert a.summary()["count"] == 5
    a.reset()
    assert a.summary()["count"] == 0
    a.add(pred[1], image[1], alpha[1], boundary[1])
    assert a.summary()["count"] == 1 and abs(a.summary()["psnr"] - float(out["psnr"][1])) <= 1e-12 * sa["psnr"]
    # an LPIPS callable rides along, frame by frame, without a read-back
    e = Evaluator("white", lpips=lambda fake, target: (fake - target).abs().mean(0))
    got = e.add(pred, image, alpha, boundary)
    assert got["lpips"].shape == (3,)
    assert abs(e.summary()["lpips"] - float((pred - got["target"]).abs().mean())) <= 1e-6


def test_add_issues_no_device_to_host_copy(cases):
    from d3ga_amd import Evaluator
    c, (pred, image, alpha, boundary) = _frames(cases)
    ev = Evaluator("black")
    ev.add(pred[0], image[0], alpha[0], boundary[0])          # the accumulator exists
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ev.add(pred, image, alpha, boundary)
        ev.add(pred[1], image[1], alpha[1], boundary[1])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert ev.summary()["count"] == 5


def test_two_calls_are_bit_identical(cases):
    from d3ga_amd import Evaluator
    c, (pred, image, alpha, boundary) = _frames(cases)
    ev = Evaluator("white")
    first, second = ev.add(pred, image, alpha, boundary), ev.add(pred, image, alpha, boundary)
    for k in OUTPUTS:
        assert torch.equal(first[k], second[k]), k


def test_captured_add_follows_its_slots(cases):
    from d3ga_amd import Evaluator
    c, (pred, image, alpha, boundary) = _frames(cases)
    slots = [t[0].clone() for t in (pred, image, alpha, boundary)]
    ev = Evaluator("white")
    eager = [ev.add(pred[i], image[i], alpha[i], boundary[i]) for i in range(3)]
    want = ev.summary()
    ev.reset()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                             # warm-up outside the capture, as torch.cuda.graph asks
        ev.add(*slots)
    torch.cuda.current_stream().wait_stream(side)
    ev.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ev.add(*slots)
    assert ev.summary()["count"] == 0                         # capturing runs nothing
    for i in range(3):
        for slot, src in zip(slots, (pred, image, alpha, boundary)):
            slot.copy_(src[i])
        graph.replay()
        for k in ("target", "ground_truth", "heatmap", "psnr"):
            assert torch.equal(out[k], eager[i][k]), (k, i)
        assert abs(float(out["ssim"]) - float(eager[i]["ssim"])) <= SSIM_BAR
    got = ev.summary()
    assert got["count"] == 3
    assert abs(got["psnr"] - want["psnr"]) <= 1e-12 * want["psnr"] and abs(got["ssim"] - want["ssim"]) <= SSIM_BAR
