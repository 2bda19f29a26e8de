"""GPU: the device half of the JPEG encoder (csrc/jpeg_encode.hip: k_jpeg_ycc, k_jpeg_fdct) against its host statement and against PIL's
own encoder bit for bit, its address and workspace checks, the round trip through both kernel pairs, the draw kernel (csrc/draw.hip)
against its host statement with the count taken from device memory, and JpegWriter with its ring of pinned buffers."""
import io
import itertools

import numpy as np
import pytest
import torch
from PIL import Image

from test_draw_cpu import CONF, NAMES, NAN, SHAPES, host, image, records
from test_jpeg_cpu import encode, picture

pytestmark = pytest.mark.gpu

# (height, width).  97 x 523 has more than 64 luma block columns (66 at 4:4:4): a block row spans waves, the sample planes span several
# workgroups of k_jpeg_ycc in both directions, and its cropped chroma plane (49 x 262 at 4:2:0) ends in one-sample tails.  8 x 8 at 4:2:0
# is the shape that shows the padding order; 1 x 1 and 7 x 9 are all edge replication; 17 x 23 and 31 x 97 have right and bottom dummies.
SIZES = [(1, 1), (7, 9), (8, 8), (17, 23), (31, 97), (97, 523)]


def bgr_of(im):
    return np.ascontiguousarray(np.asarray(im)[:, :, ::-1])


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_device_coefficients_equal_the_host_statement_and_pil(dev, size):
    from frcnn_hip import ops
    h, w = size
    for sampling, quality in itertools.product((0, 1, 2), (75, 100)):
        im = picture(w, h, seed=w * 100 + h)
        a = bgr_of(im)
        want = ops.jpeg_entropy_decode(encode(im, quality=quality, subsampling=sampling))                # PIL's coefficients
        assert torch.equal(ops.jpeg_coefs_host(a, quality, sampling), want)
        n = want.numel()
        got = ops.jpeg_coefs(torch.from_numpy(a).to(dev), quality, sampling)
        assert got.is_cuda and got.dtype == torch.uint8 and got.numel() == n
        assert torch.equal(got.cpu(), want), (size, sampling, quality, "aligned")
        # an output address that is no multiple of 4 (coefficients stored as int16), and an image at an odd address (byte loads)
        room = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device=dev)
        src = torch.zeros(a.size + 8, dtype=torch.uint8, device=dev)
        src[1:1 + a.size] = torch.from_numpy(a).reshape(-1).to(dev)
        im_odd = src[1:1 + a.size].view(h, w, 3)
        assert room[2:].data_ptr() % 4 == 2 and im_odd.data_ptr() % 2 == 1
        out = ops.jpeg_coefs(im_odd, quality, sampling, out=room[2:2 + n])
        assert torch.equal(out.cpu(), want), (size, sampling, quality, "unaligned")
        assert bool((room[:2] == 0xA5).all()) and bool((room[2 + n:] == 0xA5).all())


def test_odd_output_address_and_short_workspace_are_refused_and_nothing_runs(dev):
    import frcnn_hip
    from frcnn_hip import ops
    lib = frcnn_hip.lib()
    h, w = 33, 50
    im = picture(w, h, 2)
    im_d = torch.from_numpy(bgr_of(im)).to(dev)
    need = lib.frcnn_jpeg_workspace_bytes(w, h, 3, 2, 2)
    nbytes = lib.frcnn_jpeg_coef_bytes(w, h, 3, 2, 2)
    assert need >= 48 * 64 + 2 * 24 * 32                                 # the three MCU-padded sample planes (33 x 50: 3 x 4 MCUs)
    ws = torch.full((need,), 7, dtype=torch.uint8, device=dev)
    out = torch.full((nbytes + 16,), 9, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    args = lambda o, n: (im_d.data_ptr(), w, h, 2, 2, 75, o, ws.data_ptr(), n, st)
    assert lib.frcnn_jpeg_coefs(*args(out.data_ptr(), need - 1)) == -1    # FRCNN_E_ARG: a workspace one byte short
    assert lib.frcnn_jpeg_coefs(*args(out.data_ptr() + 1, need)) == -1    # an odd coefficient address
    assert lib.frcnn_jpeg_coefs(im_d.data_ptr(), w, h, 1, 2, 75, out.data_ptr(), ws.data_ptr(), need, st) == -3
    assert lib.frcnn_jpeg_coefs(im_d.data_ptr(), w, h, 2, 2, 0, out.data_ptr(), ws.data_ptr(), need, st) == -1
    torch.cuda.synchronize()
    assert bool((ws == 7).all()) and bool((out == 9).all())
    assert lib.frcnn_jpeg_coefs(*args(out.data_ptr(), need)) == 0
    want = ops.jpeg_entropy_decode(encode(im, quality=75, subsampling=2))
    assert torch.equal(out[:nbytes].cpu(), want) and bool((out[nbytes:] == 9).all())


@pytest.mark.parametrize("size", [(17, 23), (97, 523)], ids=lambda s: "%dx%d" % s)
def test_round_trip_through_both_kernel_pairs_equals_pil(dev, size):
    from frcnn_hip import jpeg, ops
    h, w = size
    for sampling, quality in itertools.product((0, 1, 2), (75, 100)):
        im = picture(w, h, seed=7 + sampling)
        x = torch.from_numpy(bgr_of(im)).to(dev)
        geom = ops.jpeg_encode_geom(h, w, sampling)
        back = ops.jpeg_pixels(ops.jpeg_coefs(x, quality, sampling), geom)
        theirs = encode(im, quality=quality, subsampling=sampling)
        want = np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(theirs)).convert("RGB"))[:, :, ::-1])
        assert torch.equal(back.cpu(), torch.from_numpy(want)), (size, sampling, quality)
        data = jpeg.encode_bgr(x, quality, sampling)                                 # the device path of the public entry
        assert data == jpeg.encode_bgr(x.cpu(), quality, sampling)
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[:, :, ::-1], want)


def _draw_device(dev, base, dets, cnt, odd=False, **kw):
    from utils import visualization as vis
    h, w = base.shape[:2]
    room = torch.full((base.size + 16,), 0x5A, dtype=torch.uint8, device=dev)
    off = 5 if odd else 4                                                           # (allocations are at least 256-byte aligned)
    room[off:off + base.size] = torch.from_numpy(base).reshape(-1).to(dev)
    im_d = room[off:off + base.size].view(h, w, 3)
    assert im_d.data_ptr() % 4 == off % 4
    cnt_d = torch.tensor([cnt], dtype=torch.int32, device=dev)
    vis.draw_detections(im_d, torch.from_numpy(dets).to(dev), cnt_d, NAMES, conf=CONF, **kw)
    torch.cuda.synchronize()
    assert bool((room[:off] == 0x5A).all()) and bool((room[off + base.size:] == 0x5A).all())
    return im_d.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_draw_kernel_equals_the_host_statement(dev, shape):
    h, w = shape
    base = image(h, w)
    dets, cnt = records(h, w)
    for (thickness, scale), odd in itertools.product([(2, 1), (1, 2), (5, 3)], (False, True)):
        want = host(base.copy(), dets, cnt, thickness=thickness, scale=scale)
        assert not np.array_equal(want, base)
        got = _draw_device(dev, base, dets, cnt, odd=odd, thickness=thickness, scale=scale)
        assert np.array_equal(got, want), (thickness, scale, odd)
    assert np.array_equal(_draw_device(dev, base, dets, 0), base)                    # a count of zero: untouched
    assert np.array_equal(_draw_device(dev, base, dets, 10 ** 6), host(base.copy(), dets, cnt))      # capped at the record's rows
    assert np.array_equal(_draw_device(dev, base, dets, 8), host(base.copy(), dets, 8))


def test_draw_kernel_with_more_records_than_one_staging_chunk(dev):
    """600 records of which the kernel stages 256 at a time, last chunk first: the order across chunks is the record order"""
    h, w = SHAPES[1]
    rng = np.random.RandomState(5)
    base = image(h, w)
    dets = np.zeros((640, 6), dtype=np.float32)
    x1, y1 = rng.uniform(-20, w, 640), rng.uniform(-20, h, 640)
    dets[:, 0], dets[:, 1], dets[:, 2], dets[:, 3] = x1, y1, x1 + rng.uniform(-5, 120, 640), y1 + rng.uniform(-5, 60, 640)
    dets[:, 4], dets[:, 5] = rng.uniform(0.6, 1.0, 640), rng.randint(-1, 23, 640)
    dets[rng.randint(0, 640, 20), rng.randint(0, 4, 20)] = NAN
    want = host(base.copy(), dets, 600)
    assert not np.array_equal(want, host(base.copy(), dets, 512))
    assert np.array_equal(_draw_device(dev, base, dets, 600), want)
    assert np.array_equal(_draw_device(dev, base, dets, 257, odd=True), host(base.copy(), dets, 257))


def test_writer_wraps_its_ring_of_pinned_buffers(dev, tmp_path):
    from frcnn_hip import jpeg, ops
    sizes = [(40, 30), (97, 31), (64, 48), (33, 50), (160, 120)]
    ims = [bgr_of(picture(*sizes[i % 5], seed=i)) for i in range(10)]
    wr = jpeg.JpegWriter(dev, workers=3, depth=4)
    for i, a in enumerate(ims):
        wr.submit(str(tmp_path / ("%02d.jpg" % i)), torch.from_numpy(a).to(dev), quality=85, subsampling=i % 3)
    wr.close()
    assert len(wr._slots) == 4 and all(s.buf is not None and s.buf.is_pinned() for s in wr._slots)       # 10 files through 4 buffers
    for i, a in enumerate(ims):
        data = (tmp_path / ("%02d.jpg" % i)).read_bytes()
        assert torch.equal(ops.jpeg_entropy_decode(data), ops.jpeg_coefs_host(a, 85, i % 3)), i
        assert Image.open(io.BytesIO(data)).size == (a.shape[1], a.shape[0])
    wr = jpeg.JpegWriter(dev, workers=2, depth=2)
    wr.submit(str(tmp_path / "no_such_dir" / "a.jpg"), torch.from_numpy(ims[0]).to(dev))
    with pytest.raises(OSError):
        wr.close()
