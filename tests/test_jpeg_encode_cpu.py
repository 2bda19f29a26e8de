"""CPU: the host half of the JPEG encoder (csrc/jpeg_encode_host.h) and the host statement of its coefficient stage (csrc/jpeg_math.h, the
arithmetic header the kernels of csrc/jpeg_encode.hip compile too) against PIL's own encoder -- bit for bit over the WHOLE coefficient
buffer (tables, real blocks, dummy blocks), because the rules are libjpeg's integer rules -- and the Huffman stage: the round trip through
this project's decoder and through PIL, and the bound on what it writes."""
import io
import itertools

import numpy as np
import pytest
import torch
from PIL import Image

import frcnn_hip
from frcnn_hip import jpeg, ops
from test_jpeg_cpu import encode, picture

OK, E_ARG, E_UNSUPPORTED = 0, -1, -3
SIZES = [(1, 1), (8, 8), (16, 16), (7, 9), (17, 23), (33, 50), (48, 64), (31, 97)]          # (height, width)
SAMPLING = {0: (1, 1), 1: (2, 1), 2: (2, 2)}


ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
          57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def bgr_of(im):
    return np.ascontiguousarray(np.asarray(im)[:, :, ::-1])


def test_quant_tables_equal_pil_for_every_quality():
    for q in range(1, 101):
        data = encode(picture(8, 8, 1), quality=q, subsampling=0)
        pil = Image.open(io.BytesIO(data)).quantization
        got = ops.jpeg_quant_tables(q)
        assert got.shape == (2, 64) and got.dtype == np.uint16
        # what PIL WRITES, read from its file in natural order by this project's parser ...
        written = ops.jpeg_entropy_decode(data)[:384].numpy().view(np.uint16).reshape(3, 64)
        assert np.array_equal(written[0], got[0]) and np.array_equal(written[1], got[1]) and np.array_equal(written[2], got[1]), q
        # ... and what PIL reports, entry for entry (PIL releases differ in the ORDER of the report: natural, or the file's zigzag)
        for t in (0, 1):
            assert list(pil[t]) in (got[t].tolist(), got[t][ZIGZAG].tolist()), (q, t)
    lib = frcnn_hip.lib()
    out = np.zeros(128, dtype=np.uint16)
    assert lib.frcnn_jpeg_quant_tables(0, out.ctypes.data) == E_ARG and lib.frcnn_jpeg_quant_tables(101, out.ctypes.data) == E_ARG
    assert lib.frcnn_jpeg_quant_tables(50, None) == E_ARG


@pytest.mark.parametrize("size", SIZES + [(2, 2049)], ids=lambda s: "%dx%d" % s)
def test_host_coefficients_equal_pil_over_the_whole_buffer(size):
    """(8, 8) at 4:2:0 catches the padding order (the downsampled last row is replicated, not the input rows); (2, 2049) at quality 100
    drives the largest DC values through the replacement of the quantiser's division."""
    h, w = size
    qualities = (100,) if size == (2, 2049) else (30, 75, 95, 100)
    n = 0
    for sampling, quality in itertools.product((0, 1, 2), qualities):
        im = picture(w, h, seed=w * 100 + h)
        data = encode(im, quality=quality, subsampling=sampling)
        want = ops.jpeg_entropy_decode(data)
        got = ops.jpeg_coefs_host(bgr_of(im), quality, sampling)
        assert got.dtype == torch.uint8 and got.numel() == want.numel() == ops.jpeg_coef_bytes((w, h, 3) + SAMPLING[sampling])
        assert torch.equal(got, want), (size, sampling, quality)
        n += 1
    assert n == 3 * len(qualities)


def test_the_wide_case_reaches_the_extreme_dc_values():
    """a flat white and a flat black image at quality 100: DC +-1016 / -1024, the ends of the quantiser's range"""
    for value, sampling in itertools.product((0, 255), (0, 2)):
        a = np.full((16, 32, 3), value, dtype=np.uint8)
        data = encode(Image.fromarray(a, "RGB"), quality=100, subsampling=sampling)
        assert torch.equal(ops.jpeg_coefs_host(a, 100, sampling), ops.jpeg_entropy_decode(data))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_entropy_encode_round_trip(size):
    h, w = size
    for sampling, quality in itertools.product((0, 1, 2), (30, 100)):
        im = picture(w, h, seed=w * 100 + h)
        coef = ops.jpeg_coefs_host(bgr_of(im), quality, sampling)
        geom = ops.jpeg_encode_geom(h, w, sampling)
        mine = ops.jpeg_entropy_encode(coef, geom)
        assert mine[:2] == b"\xff\xd8" and mine[-2:] == b"\xff\xd9" and mine[6:11] == b"JFIF\x00"
        assert len(mine) <= ops.jpeg_stream_bound(geom)
        assert ops.jpeg_info(mine) == (w, h, 3) + SAMPLING[sampling] + (0, 0, 0)          # no restart markers, SOF0
        assert torch.equal(ops.jpeg_entropy_decode(mine), coef)
        pil = Image.open(io.BytesIO(mine))
        assert pil.format == "JPEG" and pil.size == (w, h) and pil.mode == "RGB"
        assert not pil.info.get("progressive") and not pil.info.get("progression")        # baseline
        assert [c[1:3] for c in pil.layer] == [SAMPLING[sampling], (1, 1), (1, 1)]
        theirs = encode(im, quality=quality, subsampling=sampling)
        assert np.array_equal(np.asarray(pil.convert("RGB")), np.asarray(Image.open(io.BytesIO(theirs)).convert("RGB")))
        assert jpeg.encode_bgr(bgr_of(im), quality, sampling) == mine == jpeg.encode_bgr(torch.from_numpy(bgr_of(im)), quality, sampling)


def raw_encode(coef, geom, cap, canary=64):
    buf = np.full(cap + canary, 0xA5, dtype=np.uint8)
    n = frcnn_hip.lib().frcnn_jpeg_entropy_encode(coef.data_ptr(), geom[0], geom[1], geom[3], geom[4], buf.ctypes.data, cap)
    return n, bool((buf[cap:] == 0xA5).all()), buf[:max(n, 0)].tobytes()


def test_a_short_buffer_is_refused_without_a_stray_write():
    for (h, w), sampling in itertools.product(((17, 23), (33, 50)), (0, 1, 2)):
        geom = ops.jpeg_encode_geom(h, w, sampling)
        coef = ops.jpeg_coefs_host(bgr_of(picture(w, h, 3)), 90, sampling)
        whole = ops.jpeg_entropy_encode(coef, geom)
        n, intact, data = raw_encode(coef, geom, len(whole))
        assert n == len(whole) and intact and data == whole                           # exactly enough
        for cap in (len(whole) - 1, len(whole) - 2, len(whole) // 2, 700, 1, 0):       # inside the EOI, the scan, the headers; nothing
            n, intact, _ = raw_encode(coef, geom, cap)
            assert n == E_ARG and intact, cap
    lib = frcnn_hip.lib()
    assert lib.frcnn_jpeg_entropy_encode(coef.data_ptr(), 5, 5, 1, 2, None, 0) == E_UNSUPPORTED
    assert lib.frcnn_jpeg_stream_bound(5, 5, 1, 2) == 0 and lib.frcnn_jpeg_stream_bound(0, 5, 1, 1) == 0
    out = np.zeros(8, dtype=np.uint8)
    assert lib.frcnn_jpeg_coefs_host(out.ctypes.data, 5, 5, 1, 2, 90, out.ctypes.data) == E_UNSUPPORTED
    assert lib.frcnn_jpeg_coefs_host(out.ctypes.data, 1, 1, 1, 1, 0, out.ctypes.data) == E_ARG


def test_a_buffer_the_encoder_cannot_express_is_refused():
    """a table entry of 0 or above 255 (baseline has 8-bit tables) and an AC coefficient beyond 10 bits"""
    geom = ops.jpeg_encode_geom(8, 8, 0)
    coef = ops.jpeg_coefs_host(bgr_of(picture(8, 8, 2)), 90, 0)
    for at, value in ((5, 0), (70, 256)):
        bad = coef.clone()
        bad[:384].numpy().view(np.uint16)[at] = value
        with pytest.raises(ops.JpegError) as e:
            ops.jpeg_entropy_encode(bad, geom)
        assert e.value.rc == E_ARG
    bad = coef.clone()
    bad[384:].numpy().view(np.int16)[9] = 1024
    with pytest.raises(ops.JpegError):
        ops.jpeg_entropy_encode(bad, geom)
    bad[384:].numpy().view(np.int16)[9] = -1023
    assert torch.equal(ops.jpeg_entropy_decode(ops.jpeg_entropy_encode(bad, geom)), bad)


def test_writer_on_the_host_wraps_its_ring_and_reports_a_failed_write(tmp_path):
    """JpegWriter with device 'cpu' runs the host statement: the ring (7 files, depth 3), the file contents and the error path are the
    writer's own logic, the same on a GPU."""
    ims = [bgr_of(picture(17 + 5 * i, 23 + 3 * i, i)) for i in range(7)]
    wr = jpeg.JpegWriter("cpu", workers=3, depth=3)
    for i, a in enumerate(ims):
        wr.submit(str(tmp_path / ("%d.jpg" % i)), torch.from_numpy(a), quality=80, subsampling=i % 3)
    wr.close()
    assert len(wr._slots) == 3
    for i, a in enumerate(ims):
        data = (tmp_path / ("%d.jpg" % i)).read_bytes()
        assert data == jpeg.encode_bgr(a, 80, i % 3)
        assert torch.equal(ops.jpeg_entropy_decode(data), ops.jpeg_coefs_host(a, 80, i % 3))
    wr = jpeg.JpegWriter("cpu", workers=2, depth=2)
    wr.submit(str(tmp_path / "no_such_dir" / "a.jpg"), torch.from_numpy(ims[0]))
    with pytest.raises(OSError):
        wr.close()


def test_binding_lists_the_entries():
    from frcnn_hip import replay
    names = ["frcnn_jpeg_quant_tables", "frcnn_jpeg_coefs", "frcnn_jpeg_coefs_host", "frcnn_jpeg_stream_bound", "frcnn_jpeg_entropy_encode"]
    assert all(n in frcnn_hip.SIGNATURES for n in names)
    assert {"frcnn_jpeg_quant_tables", "frcnn_jpeg_coefs_host", "frcnn_jpeg_stream_bound", "frcnn_jpeg_entropy_encode"} <= replay.HOST_ONLY
    assert frcnn_hip.ABI_VERSION == 6
