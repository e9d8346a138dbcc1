"""The frame grid on the GPU (d3ga_amd/frame_grid.py, csrc/frame_grid.hip) against the g++ build of csrc/frame_grid_math.h
(tests/frame_grid_ref.py), bit for bit in uint8 and in float: every shape class, both kernels, the grids of test.py and
train.py, the edges of the text, the number formatted on the device, graph capture, the writer's ring and the drop-in."""
import functools

import numpy as np
import pytest
import torch

import frame_grid_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = ((1, 1), (2, 4), (3, 5), (7, 63), (8, 64), (9, 65), (5, 257))
CS, CHS, ORDERS, MODES = (1, 3, 4), (3, 4), ("rgb", "bgr"), ("save_image", "clip", None)
# the cross product thinned by a Latin square: every shape meets every C and every mode once; channels and order alternate so that
# every (C, mode), (C, channels) and (mode, order) pair appears
CASES = [(hw, CS[t], CHS[(j + t) % 2], ORDERS[(j + t // 2) % 2], MODES[(t + j) % 3]) for j, hw in enumerate(SHAPES) for t in range(3)]


def bits(t):
    """an array whose equality is equality of bits (NaN included)"""
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want):
    return np.array_equal(bits(got), bits(want))


@functools.lru_cache(maxsize=None)
def picture(c, h, w, seed=0, lo=0.0, hi=1.0):
    """a seeded (c, h, w) image on both sides; shared, never written to"""
    g = torch.Generator().manual_seed(1000 * seed + 100 * c + 7 * h + w)
    cpu = torch.rand(c, h, w, generator=g) * (hi - lo) + lo
    return cpu, cpu.to(DEV)


def poisoned(shape, dtype):
    if dtype == torch.uint8:
        return torch.full(shape, 0xAB, dtype=torch.uint8, device=DEV)
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def out_for(h, w, channels, quantize, out_layout="chw"):
    if quantize is None:
        return poisoned((channels, h, w) if out_layout == "chw" else (h, w, channels), torch.float32)
    return poisoned((h, w, channels), torch.uint8)


@pytest.mark.parametrize("hw,c,channels,order,quantize", CASES)
def test_shapes(hw, c, channels, order, quantize):
    from d3ga_amd.frame_grid import Panel, compose_grid, _layout_rows
    h, w = hw
    _, img = picture(c, h, w, lo=-0.1, hi=1.1)
    label = "Ag {:.3f}" if w >= 63 else "x"
    cell = torch.tensor([27.18281828], device=DEV) if w >= 63 else None
    rows = [[Panel(img, label, color=(0.9, 0.1, 0.4), value=cell)]]
    _, H, W = _layout_rows(rows, True)
    want = R.host_compose_rows(rows, quantize=quantize, order=order, channels=channels)
    for force in (False, True):
        out = out_for(H, W, channels, quantize)
        got, path = compose_grid(rows, quantize=quantize, order=order, channels=channels, out=out, return_path=True, force_scalar=force)
        assert got is out and same(got, want), (path, force)
        assert path == ("vector" if (w % 4 == 0 and not force) else "scalar")
    assert want.shape == ((channels, H, W) if quantize is None else (H, W, channels)) and (H % 2, W % 2) == (0, 0)


def _aligned_grid():
    from d3ga_amd.frame_grid import Panel
    cell = torch.tensor([31.0625], device=DEV)
    mk = lambda c, seed: picture(c, 12, 48, seed=seed, lo=-0.05, hi=1.05)[1]
    return [[Panel(mk(3, 1), "Prediction"), Panel(mk(1, 2), "GT sil", color=(1, 1, 1), bottom=True)],
            [Panel(mk(4, 3), "{:.3f} (dB)", color=(1, 1, 1), value=cell), Panel(mk(3, 4), "Deformed upper", thickness=1)]]


@pytest.mark.parametrize("quantize,channels,order,out_layout", [("save_image", 3, "rgb", "chw"), ("clip", 4, "bgr", "chw"),
                                                                 (None, 3, "rgb", "chw"), (None, 4, "bgr", "hwc"), (None, 3, "rgb", "hwc")])
def test_both_paths_equal_the_header(quantize, channels, order, out_layout):
    from d3ga_amd.frame_grid import Panel, compose_grid, compose_panels, _layout_rows
    rows = _aligned_grid()
    placed, H, W = _layout_rows(rows, True)
    kw = dict(quantize=quantize, order=order, channels=channels, out_layout=out_layout)
    want = R.host_compose(placed, (H, W), **kw)[0]
    got, path = compose_grid(rows, out=out_for(H, W, channels, quantize, out_layout), return_path=True, **kw)
    assert path == "vector" and same(got, want)
    got, path = compose_grid(rows, out=out_for(H, W, channels, quantize, out_layout), return_path=True, force_scalar=True, **kw)
    assert path == "scalar" and same(got, want)
    # one panel pointer 4 bytes off a 16-byte boundary
    p0 = rows[0][0]
    flat = torch.empty(p0.img.numel() + 1, device=DEV)
    shifted = flat[1:].view(p0.img.shape).copy_(p0.img)
    assert shifted.data_ptr() % 16 == 4
    rows2 = [[Panel(shifted, "Prediction"), rows[0][1]], rows[1]]
    got, path = compose_grid(rows2, out=out_for(H, W, channels, quantize, out_layout), return_path=True, **kw)
    assert path == "scalar" and same(got, want)
    # every panel one column to the right
    moved = [(p, y0, x0 + 1) for p, y0, x0 in placed]
    want1 = R.host_compose(moved, (H, W + 4), **kw)[0]
    got, path = compose_panels(moved, (H, W + 4), out=out_for(H, W + 4, channels, quantize, out_layout), return_path=True, **kw)
    assert path == "scalar" and same(got, want1)
    assert same(got[..., 1:W + 1] if (quantize is None and out_layout == "chw") else got[:, 1:W + 1], want)
    if quantize is not None:                                 # an odd pitch: rows W * channels + 1 bytes apart, the spare byte untouched
        pitch = W * channels + 1
        buf = torch.full((H, pitch), 0xAB, dtype=torch.uint8, device=DEV)
        out = buf.as_strided((H, W, channels), (pitch, channels, 1))
        got, path = compose_grid(rows, out=out, return_path=True, **kw)
        assert path == "scalar" and same(got, want) and (buf[:, -1] == 0xAB).all()
        # an even, padded pitch keeps the vector path
        pitch = W * channels + 8
        buf = torch.full((H, pitch), 0xAB, dtype=torch.uint8, device=DEV)
        got, path = compose_grid(rows, out=buf.as_strided((H, W, channels), (pitch, channels, 1)), return_path=True, **kw)
        assert path == "vector" and same(got, want) and (buf[:, W * channels:] == 0xAB).all()


def _labelled(cpu_img, text, **kw):
    return R.host_write_text(cpu_img, text, **kw)


def test_grid_of_test_py_without_ground_truth():
    """test.py:145-149, 176-182: (Prediction + 2 inputs) over (3D Means + 2 outputs), padded with 1 to even sizes, save_image."""
    from d3ga_amd.frame_grid import Panel, compose_grid
    names = [["Prediction", "Input upper", "Input lower"], ["3D Means", "Deformed upper", "Deformed lower"]]
    pics = [[picture(3, 9, 13, seed=10 * r + k) for k in range(3)] for r in range(2)]
    rows = [[Panel(pics[r][k][1], names[r][k]) for k in range(3)] for r in range(2)]
    image = torch.cat([torch.cat([_labelled(pics[r][k][0], names[r][k]) for k in range(3)], dim=2) for r in range(2)], dim=1)
    assert image.shape == (3, 18, 39)
    image = torch.nn.functional.pad(image, (0, 1, 0, 0), "constant", 1)
    want = R.torch_save_image_u8(image).permute(1, 2, 0)
    got = compose_grid(rows, out=poisoned((18, 40, 3), torch.uint8))
    assert same(got, want.contiguous())
    assert (got[:, 39] == 255).all()


def test_grid_of_test_py_with_ground_truth():
    """test.py:151-169: Ground truth, Ours and the heat map with its value label in one row of odd height and width."""
    from d3ga_amd.frame_grid import Panel, compose_grid
    (gt_c, gt), (pr_c, pr), (hm_c, hm) = picture(3, 9, 13, seed=21), picture(3, 9, 13, seed=22), picture(3, 9, 13, seed=23)
    psnr = np.float32(28.4375)
    cell = torch.tensor([float(psnr)], dtype=torch.float32, device=DEV)
    rows = [[Panel(gt, "Ground truth"), Panel(pr, "Ours"), Panel(hm, "{:.3f} (dB)", color=(1, 1, 1), value=cell)]]
    image = torch.cat([_labelled(gt_c, "Ground truth"), _labelled(pr_c, "Ours"),
                       _labelled(hm_c, f"{float(psnr):.3f} (dB)", color=(1, 1, 1))], dim=2)
    image = torch.nn.functional.pad(image, (0, 1, 0, 1), "constant", 1)
    assert image.shape == (3, 10, 40)
    got = compose_grid(rows, out=poisoned((10, 40, 3), torch.uint8))
    assert same(got, R.torch_save_image_u8(image).permute(1, 2, 0).contiguous())


def test_grid_of_train_py():
    """train.py:344-365: two rows of five HWC panels, np.clip(grid * 255, 0, 255).astype(uint8), RGB -> BGR."""
    from d3ga_amd.frame_grid import Panel, compose_grid
    names = [["Ground truth", "Heatmap {:.3f} (dB)", "GT sil", "Input upper", "Input lower"],
             ["Prediction", "3D Means", "Pred sil", "Deformed upper", "Deformed lower"]]
    psnr = np.float32(9.9995)
    cell = torch.tensor([float(psnr)], dtype=torch.float32, device=DEV)
    rows, a = [], []
    for r in range(2):
        row, line = [], []
        for k in range(5):
            cpu, dev = picture(1 if k == 2 else 3, 9, 13, seed=30 + 5 * r + k, lo=-0.2, hi=1.2)
            hwc = dev.permute(1, 2, 0)                       # the panels of train.py are (H, W, C)
            slot = "{:.3f}" in names[r][k]
            colour = (1, 1, 1) if slot else (0, 0, 0)
            row.append(Panel(hwc, names[r][k], color=colour, value=cell if slot else None, layout="hwc"))
            text = names[r][k].replace("{:.3f}", f"{float(psnr):.3f}")
            line.append(_labelled(cpu, text, color=colour).permute(1, 2, 0).numpy())
        rows.append(row)
        a.append(np.concatenate(line, axis=1))
    grid = np.concatenate(a, axis=0)
    want = R.numpy_clip_u8(grid)[:, :, ::-1]
    got, path = compose_grid(rows, quantize="clip", order="bgr", pad_even=False, out=poisoned((18, 65, 3), torch.uint8), return_path=True)
    assert path == "scalar" and same(got, np.ascontiguousarray(want))


def test_text_edges():
    from d3ga_amd.frame_grid import Panel, compose_grid
    (a_c, a), (b_c, b) = picture(3, 20, 80, seed=41), picture(3, 20, 80, seed=42)
    long_label = "W" * 40                                     # 40 cells of 6 u in a panel that holds 25
    rows = [[Panel(a, long_label, color=(1, 0, 0)), Panel(b, "")]]
    got = compose_grid(rows, quantize=None)
    want = R.host_compose_rows(rows, quantize=None)
    assert same(got, want)
    assert same(got[:, :, 80:], b_c) and not same(got[:, :, 72:80], a_c[:, :, 72:80])       # drawn to the edge, never beyond it
    # bottom=True, 64 bytes, a non-ASCII byte, an empty label
    for label, kw in (("qjy_", dict(bottom=True)), ("M" * 64, {}), ("caf\xe9 \xb5", {}), ("", {}), (b"\x00\x01", {})):
        rows = [[Panel(a, label, **kw)]]
        assert same(compose_grid(rows), R.host_compose_rows(rows)), label
    with pytest.raises(ValueError, match="65 bytes"):
        Panel(a, "M" * 65)
    text_rows = np.nonzero(R.host_alpha("qjy_", 80, 20, bottom=True).any(axis=1))[0]
    assert text_rows.min() >= 10 and not same(compose_grid([[Panel(a, "qjy_", bottom=True)]], quantize=None)[:, 10:], a_c[:, 10:])
    # white on the heat map, black on white, and pixels no image should hold -- under the text and beside it
    ugly = a_c.clone()
    ugly[:, 2:9, 10:40:5] = float("nan")
    ugly[0, 3:8, 12:40:5] = float("inf")
    ugly[1, 3:8, 13:40:5] = float("-inf")
    ugly[2, :, 14:80:5] = -0.75
    ugly[:, :, 16:80:5] = 1.5
    ugly[:, 15:, :] = torch.where(torch.rand(3, 5, 80, generator=torch.Generator().manual_seed(5)) < 0.3, float("nan"), 2.0)
    white = torch.ones(3, 20, 80)
    for cpu, colour in ((ugly, (1, 1, 1)), (ugly, (0, 0, 0)), (white, (0, 0, 0)), (a_c, (1, 1, 1))):
        for quantize in ("save_image", "clip", None):
            rows = [[Panel(cpu.to(DEV), "Heat 0.5", color=colour)]]
            assert same(compose_grid(rows, quantize=quantize), R.host_compose_rows(rows, quantize=quantize)), (colour, quantize)
    black = compose_grid([[Panel(white.to(DEV), "Heat", color=(0, 0, 0))]])
    assert black.min() < 128 and black.max() == 255          # black text on white darkens it


VALUES = (0.0625, 0.1875, -0.0625, 2.0625, 9.9995, 0.9996, 99.99951, 0.0, -0.0, float("inf"), float("-inf"), float("nan"), 1e-45,
          31.4159, -7.25, 123456.789, 2e6)


def test_number_formatted_on_the_device():
    from d3ga_amd.frame_grid import Panel, compose_grid
    _, img = picture(3, 16, 160, seed=50)
    cell = torch.zeros(1, device=DEV)
    for v in VALUES:
        cell.fill_(v)
        text = R.py_format(v)
        assert text == f"{float(np.float32(v)):.3f}" or abs(v) >= 1e6
        got = compose_grid([[Panel(img, "{:.3f} (dB)", color=(1, 1, 1), value=cell)]])
        static = compose_grid([[Panel(img, f"{text} (dB)", color=(1, 1, 1))]])
        assert torch.equal(got, static), v
    assert not torch.equal(got, compose_grid([[Panel(img, "0.000 (dB)", color=(1, 1, 1))]]))


def test_capture_follows_the_panel_and_the_cell():
    from d3ga_amd.frame_grid import Panel, compose_grid
    img = picture(3, 12, 48, seed=60)[1].clone()
    other = picture(1, 12, 48, seed=61)[1]
    cell = torch.tensor([20.5], device=DEV)
    rows = [[Panel(img, "{:.3f} (dB)", value=cell), Panel(other, "sil")]]
    out = poisoned((12, 96, 3), torch.uint8)
    compose_grid(rows, out=out)                              # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        compose_grid(rows, out=out)                          # a synchronisation or an allocation in here would fail the capture
    img.copy_(picture(3, 12, 48, seed=62)[1])
    cell.fill_(-3.0625)
    out.fill_(0xAB)
    graph.replay()
    eager = compose_grid(rows)
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    assert same(eager, R.host_compose_rows(rows))


def test_grid_writer():
    from d3ga_amd.frame_grid import GridWriter, to_uint8
    imgs = [to_uint8(picture(3, 9, 13, seed=70 + i)[1]) for i in range(3)]
    w = GridWriter(depth=2)
    h0, h1 = w.submit(imgs[0]), w.submit(imgs[1])            # two in flight
    assert np.array_equal(h1.numpy(), imgs[1].cpu().numpy()) and np.array_equal(h0.numpy(), imgs[0].cpu().numpy())
    w = GridWriter(depth=2)
    handles = [w.submit(t) for t in imgs]                    # the third waits for the first and hands it over, it does not overwrite it
    assert handles[0].done()
    for h, t in zip(handles, imgs):
        assert np.array_equal(h.numpy(), t.cpu().numpy()) and h.numpy().shape == (9, 13, 3)
    bigger = to_uint8(picture(4, 10, 20, seed=75)[1])        # a slot grows with what it is given; RGBA keeps its alpha
    assert bigger.shape == (10, 20, 4) and np.array_equal(w.submit(bigger).numpy(), bigger.cpu().numpy())
    assert same(bigger, R.torch_save_image_u8(picture(4, 10, 20, seed=75)[0]).permute(1, 2, 0).contiguous())


def test_grid_writer_with_a_save_pool():
    """The documented use: handle.numpy() in the save pool's threads while the frame loop keeps submitting into a ring of
    depth 2 that wraps 60 times.  Every image arrives whole and is its own; the ring ends with no stale owner."""
    from concurrent.futures import ThreadPoolExecutor
    from d3ga_amd.frame_grid import GridWriter
    n, shape = 120, (96, 512, 3)
    base = (torch.arange(shape[0] * shape[1] * shape[2], device=DEV) % 251).to(torch.uint8).view(shape)
    frames = [base + (i % 200) for i in range(n)]            # uint8 wraps: image i is known from its first byte, yet no two rows agree
    want = [f.cpu().numpy() for f in frames]
    torch.cuda.synchronize()
    w = GridWriter(depth=2)

    def save(handle):                                        # what the save pool runs
        first = handle.numpy()
        return first.copy(), handle.numpy() is first, handle.done()

    with ThreadPoolExecutor(4) as pool:
        futures = [pool.submit(save, w.submit(f)) for f in frames]
        got = [f.result() for f in futures]
    for i, (image, stable, done) in enumerate(got):
        assert np.array_equal(image, want[i]), i
        assert stable and done
    assert all(o is None for o in w._owners)
    # handles nobody takes until the end: the ring hands each over as it wraps, all stay intact
    handles = [w.submit(f) for f in frames[:9]]
    with ThreadPoolExecutor(3) as pool:
        late = list(pool.map(lambda h: h.numpy(), handles))
    assert all(np.array_equal(a, b) for a, b in zip(late, want[:9]))


def test_write_text_is_a_drop_in():
    from d3ga_amd.frame_grid import write_text
    cpu, img = picture(3, 40, 373, seed=80, lo=-0.5, hi=1.5)
    cpu = cpu.clone()
    cpu[:, 30:, ::7] = -0.0                                  # a sign bit a blend with zero coverage would lose
    img = cpu.to(DEV)
    before = img.clone()
    out = write_text(img, "Prediction", fontColor=(0, 0, 0))
    assert out.dtype == torch.float32 and out.shape == img.shape and out.data_ptr() != img.data_ptr()
    assert torch.equal(img.view(torch.int32), before.view(torch.int32))
    assert same(out, R.host_write_text(cpu, "Prediction"))
    u = float(R.unit(373))
    base = R.baseline(np.float32(u), 40, False)
    y0, y1 = int(np.floor(base - 8 * u)), int(np.ceil(base + u)) + 1
    x0, x1 = int(np.floor(15 - u)), int(np.ceil(15 + 61 * u)) + 1
    box = torch.zeros(40, 373, dtype=torch.bool)
    box[max(y0, 0):y1, max(x0, 0):x1] = True
    assert same(out.cpu()[:, ~box], cpu[:, ~box]) and not same(out.cpu()[:, box], cpu[:, box])
    hwc = write_text(img.permute(1, 2, 0), "Prediction", layout="hwc")
    assert hwc.shape == (40, 373, 3) and torch.equal(hwc.permute(2, 0, 1).view(torch.int32), out.view(torch.int32))
    thin = write_text(img, "Prediction", thickness=1)
    assert not torch.equal(thin, out)
    with pytest.raises(TypeError, match="compose_grid"):
        write_text(cpu.numpy(), "Prediction")
