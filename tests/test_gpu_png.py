"""The PNG encoder on the GPU (d3ga_amd/png.py, csrc/png.hip) against the g++ build of csrc/png_math.h and the independent
decoder (tests/png_ref.py): every case of the host tests byte for byte, determinism, graph capture, the untouched tail of the
buffer, the writer's ring, the save_image drop-in and every refusal."""
import numpy as np
import pytest
import torch

import png_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def on_device(img):
    """the same pixels and the same row pitch on the GPU"""
    H, W, C, pitch = R.image_pitch(img)
    base = torch.full((H * pitch,), 0x5A, dtype=torch.uint8, device=DEV)
    view = base.as_strided((H, W, C), (pitch, C, 1))
    view.copy_(torch.from_numpy(np.ascontiguousarray(img)))
    return view


def whole_buffer(buf):
    """(length, every byte behind the length word) after a synchronising read-back"""
    host = buf.buffer.cpu().numpy()
    return int(host[:8].view(np.uint64)[0]), host[8:]


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_kernel_bytes_equal_the_host_build(name):
    from d3ga_amd import PngBuffer, encode_png, png_bytes
    _, img, f, rows = R.CASES[R.CASE_IDS.index(name)]
    h = R.host_case(name)
    dev = on_device(img)
    assert dev.stride(0) == img.strides[0]
    H, W, C = img.shape
    buf = PngBuffer(H, W, C, rows)
    assert buf.capacity == h.capacity
    buf.buffer.fill_(0xAB)
    assert encode_png(dev, filter=f, rows_per_strip=rows, out=buf) is buf
    n, data = whole_buffer(buf)
    assert n <= buf.capacity
    got = data[:n].tobytes()
    d = R.decode(got)
    assert (d.image == img).all(), "the decoded image is the input"
    assert got == h.data, "the kernels give the g++ build's bytes"
    assert (data[n:] == 0xAB).all(), "bytes at and beyond the length are untouched"
    assert png_bytes(buf) == got
    assert png_bytes(encode_png(dev, filter=f, rows_per_strip=rows)) == got, "a second call, into a fresh buffer"


def test_capture_follows_the_image():
    from d3ga_amd import PngBuffer, encode_png, png_bytes
    first = (R.ramp(33, 17, 4) + (R.noise(33, 17, 4, 3) >> 6)).astype(np.uint8)
    second = R.noise(33, 17, 4, 21)
    img = on_device(first)
    buf = PngBuffer(33, 17, 4, 2)
    encode_png(img, out=buf)                                 # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        encode_png(img, out=buf)                             # a synchronisation or an allocation in here would fail the capture
    img.copy_(torch.from_numpy(second).to(DEV))
    buf.buffer.fill_(0xAB)
    graph.replay()
    torch.cuda.synchronize()
    n, data = whole_buffer(buf)
    replayed = data[:n].tobytes()
    assert (data[n:] == 0xAB).all()
    eager = png_bytes(encode_png(img, rows_per_strip=2))
    assert replayed == eager == R.host_encode(second, "adaptive", 2).data
    assert (R.decode(replayed).image == second).all()


def test_writer_hands_out_the_file():
    from d3ga_amd import GridWriter, PngBuffer, encode_png, png_bytes
    writer = GridWriter(depth=2)
    imgs = [R.noise(9, 11, 3, 30 + k) for k in range(3)]
    bufs = [encode_png(on_device(im), out=PngBuffer(9, 11, 3)) for im in imgs]
    handles = [writer.submit_png(b) for b in bufs]            # three into a ring of two: the first is taken out for its handle
    for im, b, hd in zip(imgs, bufs, handles):
        assert hd.tobytes() == png_bytes(b) == R.host_encode(im).data
        assert hd.done()
    with pytest.raises(TypeError, match="PngBuffer"):
        writer.submit_png(bufs[0].buffer)


def test_save_image_is_to_uint8_then_the_encoder(tmp_path):
    from d3ga_amd import save_image, to_uint8
    g = torch.Generator().manual_seed(5)
    img = (torch.rand(3, 9, 11, generator=g) * 1.2 - 0.1).to(DEV)
    path = tmp_path / "frame.png"
    save_image(img, str(path))
    d = R.decode(path.read_bytes())
    want = to_uint8(img).cpu().numpy()
    assert d.image.shape == (9, 11, 3) and (d.image == want).all()
    save_image(to_uint8(img), str(path))                      # a uint8 (H, W, C) image is written as it is
    assert (R.decode(path.read_bytes()).image == want).all()


def test_refusals_raise_before_any_launch():
    from d3ga_amd import PngBuffer, encode_png
    img = on_device(R.noise(9, 11, 3, 4))
    buf = PngBuffer(9, 11, 3)
    buf.storage.fill_(0xAB)

    def refused(exc, match, *a, **kw):
        with pytest.raises(exc, match=match):
            encode_png(*a, **kw)
    refused(ValueError, "img_u8 is on cpu", img.cpu(), out=buf)
    refused(TypeError, "img_u8 must be uint8", img.float(), out=buf)
    refused(TypeError, "img_u8", img.cpu().numpy(), out=buf)
    refused(ValueError, "img_u8 must be \\(H, W, C\\)", img[0], out=buf)
    refused(ValueError, "C=2", img[:, :, :2].contiguous(), out=buf)
    refused(ValueError, "img_u8 is empty", img[:0], out=buf)
    refused(ValueError, "img_u8 is empty", img[:, :0], out=buf)
    refused(ValueError, "strides", img.permute(1, 0, 2), out=buf)
    refused(ValueError, "strides", img[:, ::2], out=buf)
    refused(ValueError, "strides", img[:, :, :1], out=buf)                      # C = 1 inside RGB pixels: not dense
    refused(ValueError, "filter", img, filter=5, out=buf)
    refused(ValueError, "filter", img, filter="paeth", out=buf)
    refused(ValueError, "rows_per_strip", img, rows_per_strip=-1, out=buf)
    refused(TypeError, "rows_per_strip", img, rows_per_strip=1.5, out=buf)
    refused(TypeError, "out must be a PngBuffer", img, out=buf.buffer)
    refused(ValueError, "out is too small", img, out=PngBuffer(8, 11, 3))
    refused(ValueError, "out is too small", img, rows_per_strip=1, out=buf)      # more strips than the buffer was sized for
    for args in ((0, 4, 3), (4, 0, 3), (4, 4, 2), (4, (2 ** 31 - 1) // 4 + 1, 4), (2 ** 31, 4, 1)):
        with pytest.raises(ValueError, match="PngBuffer"):
            PngBuffer(*args)
    torch.cuda.synchronize()
    assert bool((buf.storage == 0xAB).all()), "a refused call wrote nothing: no launch reached the buffer"
