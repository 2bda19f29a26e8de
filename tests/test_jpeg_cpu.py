"""CPU: the host half of the JPEG path (csrc/jpeg_host.h) and the host statement of its pixel stage (csrc/jpeg_math.h, the arithmetic
header the kernels compile too) against PIL -- bit for bit, because the rules are libjpeg's integer rules --, the geometry and size
queries, the streams the decoder must hand back to PIL, and damaged streams: whatever the bytes are, the return value is one of three
codes, nothing is written behind the coefficient buffer and the process survives."""
import ctypes
import io
import itertools

import numpy as np
import pytest
import torch
from PIL import Image

import frcnn_hip
from frcnn_hip import jpeg, ops

OK, E_ARG, E_UNSUPPORTED = 0, -1, -3
SIZES = [(1, 1), (8, 8), (7, 9), (17, 23), (33, 50), (48, 64), (31, 97)]          # (height, width)


def picture(w, h, seed, mode="RGB"):
    """seeded smooth-plus-noise image"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    chans = []
    for c in range(3):
        smooth = 128 + 90 * np.sin(xx / (3.0 + c) + c) * np.cos(yy / (5.0 - c)) + 30 * np.sin((xx + yy) / 11.0)
        chans.append(smooth + rng.randn(h, w) * 12)
    a = np.clip(np.stack(chans, axis=2), 0, 255).astype(np.uint8)
    im = Image.fromarray(a, "RGB")
    return im if mode == "RGB" else im.convert(mode)


def encode(im, **kw):
    f = io.BytesIO()
    im.save(f, "JPEG", **kw)
    return f.getvalue()


def pil_pixels(data):
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[:, :, ::-1])


def raw_decode(data, coef_bytes, canary=64):
    """frcnn_jpeg_entropy_decode into a buffer of coef_bytes followed by a canary -> (rc, canary intact)"""
    buf = np.full(coef_bytes + canary, 0xA5, dtype=np.uint8)
    rc = frcnn_hip.lib().frcnn_jpeg_entropy_decode(data, len(data), buf.ctypes.data, coef_bytes)
    return rc, bool((buf[coef_bytes:] == 0xA5).all())


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_host_pixels_equal_pil_bit_for_bit(size):
    h, w = size
    n = 0
    for sampling, quality, restart, optimize in itertools.product((0, 1, 2, "L"), (30, 75, 95, 100), (0, 3), (False, True)):
        im = picture(w, h, seed=w * 100 + h, mode="L" if sampling == "L" else "RGB")
        kw = dict(quality=quality, restart_marker_blocks=restart, optimize=optimize)
        if sampling != "L":
            kw["subsampling"] = sampling
        data = encode(im, **kw)
        geom = ops.jpeg_info(data)
        assert geom[:2] == (w, h) and geom[2] == (1 if sampling == "L" else 3)
        assert geom[5] == restart, "PIL writes restart markers"
        got = ops.jpeg_pixels_host(ops.jpeg_entropy_decode(data), geom)
        assert np.array_equal(got, pil_pixels(data)), (size, sampling, quality, restart, optimize)
        n += 1
    assert n == 64


def test_geometry_and_sizes():
    lib = frcnn_hip.lib()
    for (sampling, hs, vs), (w, h) in itertools.product(((0, 1, 1), (1, 2, 1), (2, 2, 2)), ((33, 50), (17, 23), (48, 64))):
        data = encode(picture(w, h, 5), quality=75, subsampling=sampling, restart_marker_blocks=2)
        assert ops.jpeg_info(data) == (w, h, 3, hs, vs, 2, 0, 0)
        mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
        blocks = mx * hs * my * vs + 2 * mx * my
        assert lib.frcnn_jpeg_coef_bytes(w, h, 3, hs, vs) == 384 + 2 * 64 * blocks == ops.jpeg_coef_bytes((w, h, 3, hs, vs))
        rc, intact = raw_decode(data, 384 + 128 * blocks)
        assert rc == OK and intact
        rc, intact = raw_decode(data, 384 + 128 * blocks - 1)                      # one byte short: refused, nothing written behind it
        assert rc == E_ARG and intact
    data = encode(picture(31, 97, 6, "L"), quality=75)
    assert ops.jpeg_info(data) == (31, 97, 1, 1, 1, 0, 0, 0)
    assert lib.frcnn_jpeg_coef_bytes(31, 97, 1, 1, 1) == 384 + 128 * 4 * 13
    # the layout: quantisation tables in natural order first (quality 100: all ones), then the coefficients
    coef = ops.jpeg_entropy_decode(encode(picture(8, 8, 7), quality=100, subsampling=0))
    assert coef.numel() == 384 + 3 * 128 and np.array_equal(coef[:384].numpy().view(np.uint16), np.ones(192, dtype=np.uint16))
    for bad in ((0, 5, 3, 1, 1), (5, 0, 3, 1, 1), (5, 5, 2, 1, 1), (5, 5, 3, 1, 2), (5, 5, 3, 4, 1), (5, 5, 1, 2, 2), (70000, 5, 3, 1, 1)):
        assert lib.frcnn_jpeg_coef_bytes(*bad) == 0 and lib.frcnn_jpeg_workspace_bytes(*bad) == 0, bad
    out = np.zeros((5, 5, 3), dtype=np.uint8)
    assert lib.frcnn_jpeg_pixels_host(coef.data_ptr(), 5, 5, 3, 1, 2, out.ctypes.data) == E_UNSUPPORTED


def unsupported_streams():
    rgb = picture(40, 30, 9)
    png = io.BytesIO()
    rgb.save(png, "PNG")
    return {"progressive": encode(rgb, quality=80, progressive=True), "cmyk": encode(rgb.convert("CMYK"), quality=80), "png": png.getvalue()}


def test_unsupported_streams_go_back_to_pil(tmp_path):
    lib = frcnn_hip.lib()
    info = (ctypes.c_int * 8)()
    for name, data in unsupported_streams().items():
        assert lib.frcnn_jpeg_info(data, len(data), info) == E_UNSUPPORTED, name
        rc, intact = raw_decode(data, 1 << 16)
        assert rc == E_UNSUPPORTED and intact, name
        with pytest.raises(ops.JpegError) as e:
            ops.jpeg_info(data)
        assert e.value.rc == E_UNSUPPORTED
        want = pil_pixels(data)
        got = jpeg.decode_bgr(data, "cpu")                                             # bytes
        assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), want), name
        path = tmp_path / (name + ".img")
        path.write_bytes(data)
        assert np.array_equal(jpeg.decode_bgr(str(path), "cpu").numpy(), want), name    # file
    for data in (b"", b"\xff", b"GIF89a", b"\x00" * 64):
        assert lib.frcnn_jpeg_info(data, len(data), info) == E_UNSUPPORTED


def test_supported_stream_on_the_host_and_ordered_prefetch(tmp_path):
    """decode_bgr / JpegPrefetcher with device 'cpu' run the host statement: the order, the ring of buffers (it wraps: 7 files, depth 3) and the
    PIL fallback inside the stream are the prefetcher's own logic, the same on a GPU."""
    items = [encode(picture(17 + 5 * i, 23 + 3 * i, i), quality=75, subsampling=i % 3, restart_marker_blocks=i % 2) for i in range(5)]
    u = unsupported_streams()
    items.insert(2, u["progressive"])
    items.insert(5, u["png"])
    paths = []
    for i, d in enumerate(items):
        p = tmp_path / ("%d.jpg" % i)
        p.write_bytes(d)
        paths.append(str(p))
    assert np.array_equal(jpeg.decode_bgr(paths[0], "cpu").numpy(), pil_pixels(items[0]))
    got = list(jpeg.JpegPrefetcher(paths, "cpu", workers=3, depth=3))
    assert len(got) == len(items)
    for g, d in zip(got, items):
        assert np.array_equal(g.numpy(), pil_pixels(d))
    # a damaged stream is PIL's business as before: its pixels or its error
    broken = items[0][:len(items[0]) // 2]
    with pytest.raises(ops.JpegError) as e:
        ops.jpeg_entropy_decode(broken)
    assert e.value.rc == E_ARG
    with pytest.raises(OSError):
        pil_pixels(broken)
    with pytest.raises(OSError):
        jpeg.decode_bgr(broken, "cpu")


def test_damaged_streams_are_refused_without_a_stray_write():
    data = encode(picture(50, 33, 11), quality=75, subsampling=2, restart_marker_blocks=3)       # 33 x 50 (h x w)
    geom = ops.jpeg_info(data)
    assert geom[3:6] == (2, 2, 3)                          # 4:2:0, a restart marker every 3 MCUs
    nbytes = ops.jpeg_coef_bytes(geom)
    sos = data.index(b"\xff\xda")
    scan = sos + 2 + ((data[sos + 2] << 8) | data[sos + 3])
    lib = frcnn_hip.lib()
    info = (ctypes.c_int * 8)()
    seen = set()
    for cut in range(0, len(data), 7):
        d = data[:cut]
        rc, intact = raw_decode(d, nbytes)
        assert rc in (OK, E_ARG, E_UNSUPPORTED) and intact, cut
        assert lib.frcnn_jpeg_info(d, len(d), info) in (OK, E_ARG, E_UNSUPPORTED)
        if cut < len(data) - 16:
            assert rc != OK, cut                           # (a cut inside the last bytes may lose only the EOI marker)
        seen.add(rc)
    rng = np.random.RandomState(4)
    for _ in range(300):
        d = bytearray(data)
        d[rng.randint(scan, len(data))] = rng.randint(0, 256)
        d = bytes(d)
        rc, intact = raw_decode(d, nbytes)
        assert rc in (OK, E_ARG, E_UNSUPPORTED) and intact
        seen.add(rc)
    assert seen == {OK, E_ARG, E_UNSUPPORTED}              # an empty prefix is no JPEG, a cut scan is damaged, some corruptions still decode


def test_binding_lists_the_entries():
    from frcnn_hip import replay
    names = ["frcnn_jpeg_info", "frcnn_jpeg_coef_bytes", "frcnn_jpeg_entropy_decode", "frcnn_jpeg_pixels_host", "frcnn_jpeg_workspace_bytes",
             "frcnn_jpeg_pixels"]
    assert all(n in frcnn_hip.SIGNATURES for n in names)
    assert {"frcnn_jpeg_info", "frcnn_jpeg_entropy_decode", "frcnn_jpeg_pixels_host"} <= replay.HOST_ONLY
    assert frcnn_hip.ABI_VERSION == 6
    from model.config import cfg
    assert cfg.HIP.JPEG_DEVICE is False
