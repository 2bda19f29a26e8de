"""CPU: the host half of the TensorBoard summaries (frcnn_hip/summary.py, frcnn_summary_limits): the bucket limits, the event-file
framing and encoders against an INDEPENDENT decoder (google.protobuf messages built from descriptors written here, a bitwise crc32c
written here), the bucket compression, the numpy statement of the statistics that tests/test_summary_gpu.py holds the kernel to."""
import math
import struct

import numpy as np
import pytest

from frcnn_hip import ops, summary


# ---- independent reader --------------------------------------------------------------------------------------------------------------
def crc32c_bitwise(data):
    c = 0xFFFFFFFF
    for b in data:
        c ^= b
        for _ in range(8):
            c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1
    return c ^ 0xFFFFFFFF


def masked(c):
    return ((((c >> 15) | (c << 17)) & 0xFFFFFFFF) + 0xa282ead8) & 0xFFFFFFFF


def read_records(path):
    """payloads of a TFRecord file; both crc fields of every record are verified with the bitwise crc above"""
    data = open(path, "rb").read()
    pos, out = 0, []
    while pos < len(data):
        (n,) = struct.unpack_from("<Q", data, pos)
        (c1,) = struct.unpack_from("<I", data, pos + 8)
        if c1 != masked(crc32c_bitwise(data[pos:pos + 8])):
            raise IOError("length crc mismatch at %d" % pos)
        payload = data[pos + 12:pos + 12 + n]
        if len(payload) != n:
            raise IOError("truncated record at %d" % pos)
        (c2,) = struct.unpack_from("<I", data, pos + 12 + n)
        if c2 != masked(crc32c_bitwise(payload)):
            raise IOError("payload crc mismatch at %d" % pos)
        out.append(payload)
        pos += 16 + n
    return out


def event_class():
    """tensorflow.Event (with Summary, Summary.Value, Summary.Image, HistogramProto) as google.protobuf builds it from a descriptor."""
    from google.protobuf import descriptor_pb2, descriptor_pool
    try:
        from google.protobuf import message_factory
        get_class = message_factory.GetMessageClass
    except (ImportError, AttributeError):                      # older protobuf
        from google.protobuf import message_factory
        get_class = lambda d: message_factory.MessageFactory().GetPrototype(d)
    F = descriptor_pb2.FieldDescriptorProto
    fd = descriptor_pb2.FileDescriptorProto(name="summary_test.proto", package="tbtest", syntax="proto3")

    def msg(name, fields, parent=None):
        m = (parent.nested_type if parent is not None else fd.message_type).add(name=name)
        for fname, num, typ, label, tname in fields:
            f = m.field.add(name=fname, number=num, type=typ, label=label)
            if tname:
                f.type_name = tname
        return m
    O, R = F.LABEL_OPTIONAL, F.LABEL_REPEATED
    msg("HistogramProto", [("min", 1, F.TYPE_DOUBLE, O, None), ("max", 2, F.TYPE_DOUBLE, O, None), ("num", 3, F.TYPE_DOUBLE, O, None),
                           ("sum", 4, F.TYPE_DOUBLE, O, None), ("sum_squares", 5, F.TYPE_DOUBLE, O, None),
                           ("bucket_limit", 6, F.TYPE_DOUBLE, R, None), ("bucket", 7, F.TYPE_DOUBLE, R, None)])
    s = msg("Summary", [("value", 1, F.TYPE_MESSAGE, R, ".tbtest.Summary.Value")])
    msg("Image", [("height", 1, F.TYPE_INT32, O, None), ("width", 2, F.TYPE_INT32, O, None), ("colorspace", 3, F.TYPE_INT32, O, None),
                  ("encoded_image_string", 4, F.TYPE_BYTES, O, None)], parent=s)
    msg("Value", [("tag", 1, F.TYPE_STRING, O, None), ("simple_value", 2, F.TYPE_FLOAT, O, None),
                  ("image", 4, F.TYPE_MESSAGE, O, ".tbtest.Summary.Image"), ("histo", 5, F.TYPE_MESSAGE, O, ".tbtest.HistogramProto")], parent=s)
    msg("Event", [("wall_time", 1, F.TYPE_DOUBLE, O, None), ("step", 2, F.TYPE_INT64, O, None), ("file_version", 3, F.TYPE_STRING, O, None),
                  ("summary", 5, F.TYPE_MESSAGE, O, ".tbtest.Summary")])
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    return get_class(pool.FindMessageTypeByName("tbtest.Event"))


def expand_buckets(bucket_limit, bucket, limits):
    """a reader's view of a written HistogramProto: dense counts over `limits`"""
    index = {float(v): i for i, v in enumerate(limits)}
    dense = np.zeros((len(limits),), dtype=np.int64)
    for lim, c in zip(bucket_limit, bucket):
        dense[index[float(lim)]] = int(c)
    return dense


def parse_events(path):
    Event = event_class()
    out = []
    for payload in read_records(path):
        e = Event()
        e.ParseFromString(payload)
        out.append(e)
    return out


# ---- tests ---------------------------------------------------------------------------------------------------------------------------
def python_limits():
    pos = []
    v = 1e-12
    while v < 1e20:
        pos.append(v)
        v *= 1.1
    assert len(pos) == 774
    pos.append(np.finfo(np.float64).max)
    return np.array([-x for x in reversed(pos)] + [0.0] + pos, dtype=np.float64)


def test_limit_table_is_tensorflows_bit_for_bit():
    got = ops.summary_limits()
    want = python_limits()
    assert got.shape == (1551,) and got.dtype == np.float64
    assert got.tobytes() == want.tobytes()                                 # bit for bit: the product chain, never pow
    assert np.all(np.diff(got) > 0) and got[775] == 0.0 and not np.signbit(got[775])
    assert got[0] == -np.finfo(np.float64).max and got[1550] == np.finfo(np.float64).max and got[776] == 1e-12
    assert not np.allclose(want[776:1550], 1e-12 * np.power(1.1, np.arange(774)), rtol=0, atol=0)      # (pow is NOT the same table)
    # no float32 equals a non-zero limit: the bracketing pairs of the GPU test always straddle
    inside = want[(np.abs(want) <= np.finfo(np.float32).max) & (want != 0)]
    assert inside.size == 1548 and not np.any(inside.astype(np.float32).astype(np.float64) == inside)


def test_numpy_statement_on_hand_made_values():
    f32 = np.float32
    fmax = np.finfo(np.float32).max
    vals = [0.0, -0.0, 1e-13, -1e-13, f32(1e-12), 1.0, f32(1.1), fmax, -fmax]
    want = [776, 776, 776, 775, 776, 1066, 1067, 1550, 1]
    limits = ops.summary_limits()
    for v, b in zip(vals, want):
        st = summary.reference_stats(np.array([v], dtype=np.float32), limits)
        assert int(np.argmax(st["counts"])) == b and st["counts"].sum() == 1, (v, b)
    x = np.array(vals + [np.nan, np.inf, -np.inf], dtype=np.float32)
    st = summary.reference_stats(x, limits)
    assert st["num"] == 12 and st["n_zero"] == 2 and st["n_nonfinite"] == 3 and st["counts"].sum() == 9
    assert st["min"] == -float(fmax) and st["max"] == float(fmax)
    d = x[:9].astype(np.float64)
    assert st["sum"] == math.fsum(d.tolist()) and st["sum_squares"] == math.fsum((d * d).tolist())
    assert summary.zero_fraction(st) == 2 / 12
    empty = summary.reference_stats(np.zeros((0,), dtype=np.float32), limits)
    assert empty["num"] == 0 and empty["counts"].sum() == 0 and empty["min"] == np.finfo(np.float64).max and empty["sum"] == 0.0


def test_bucket_compression_round_trip():
    limits = ops.summary_limits()
    rng = np.random.RandomState(0)
    cases = [np.zeros(1551, dtype=np.int64)]
    for density in (0.01, 0.3, 1.0):
        c = (rng.rand(1551) < density) * rng.randint(1, 1000, size=1551)
        cases.append(c.astype(np.int64))
    one = np.zeros(1551, dtype=np.int64)
    one[776] = 12345
    last = np.zeros(1551, dtype=np.int64)
    last[1550], last[0] = 7, 3
    cases += [one, last]
    for dense in cases:
        lim, cnt = summary.compress_buckets(dense, limits)
        assert len(lim) == len(cnt) >= 1 and np.all(np.diff(lim) > 0)
        assert not any(a == 0 and b == 0 for a, b in zip(cnt[:-1], cnt[1:]))            # every run of empty buckets is ONE entry
        assert np.array_equal(expand_buckets(lim, cnt, limits), dense)
        assert sum(cnt) == dense.sum()
    lim, cnt = summary.compress_buckets(one, limits)
    assert lim == [limits[775], limits[776], limits[1550]] and cnt == [0.0, 12345.0, 0.0]      # a run carries its LAST limit


def test_event_file_round_trip_against_protobuf(tmp_path):
    limits = ops.summary_limits()
    rng = np.random.RandomState(1)
    x = np.concatenate([rng.randn(5000), np.zeros(700)]).astype(np.float32)
    st = summary.reference_stats(x, limits)
    rgb = (rng.rand(13, 17, 3) * 255).astype(np.uint8)
    w = summary.FileWriter(str(tmp_path))
    w.add_summary(summary.scalar("total_loss", 1.25) + summary.histogram("TRAIN/w", st, limits) + summary.image("GROUND_TRUTH", rgb), 7)
    w.add_summary(summary.scalar("total_loss", 0.5), 8)
    w.flush()
    w.close()
    import os
    (name,) = os.listdir(str(tmp_path))
    assert name.startswith("events.out.tfevents.") and name == os.path.basename(w.path)
    ev = parse_events(w.path)
    assert len(ev) == 3
    assert ev[0].file_version == "brain.Event:2" and ev[0].step == 0 and ev[0].wall_time > 1e9 and len(ev[0].summary.value) == 0
    assert ev[1].step == 7 and ev[2].step == 8 and ev[1].wall_time >= ev[0].wall_time
    sc, hi, im = ev[1].summary.value
    assert sc.tag == "total_loss" and sc.simple_value == 1.25 and ev[2].summary.value[0].simple_value == 0.5
    assert hi.tag == "TRAIN/w"
    h = hi.histo
    assert (h.min, h.max, h.num, h.sum, h.sum_squares) == (st["min"], st["max"], float(st["num"]), st["sum"], st["sum_squares"])
    assert np.array_equal(expand_buckets(list(h.bucket_limit), list(h.bucket), limits), st["counts"])
    assert sum(h.bucket) == x.size and h.bucket[list(h.bucket_limit).index(1e-12)] >= 700
    assert im.tag.startswith("GROUND_TRUTH") and (im.image.height, im.image.width, im.image.colorspace) == (13, 17, 3)
    import io
    from PIL import Image
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(im.image.encoded_image_string))), rgb)
    # a flipped payload byte is detected (by the reader's own crc)
    raw = bytearray(open(w.path, "rb").read())
    raw[len(raw) // 2] ^= 0x10
    bad = tmp_path / "damaged"
    bad.write_bytes(bytes(raw))
    with pytest.raises(IOError):
        read_records(str(bad))
    raw = bytearray(open(w.path, "rb").read())
    raw[3] ^= 0x01                                                       # ... and a damaged length field
    bad.write_bytes(bytes(raw))
    with pytest.raises(IOError):
        read_records(str(bad))


def test_non_finite_tensor_raises_with_its_tag():
    limits = ops.summary_limits()
    for v in (np.nan, np.inf, -np.inf):
        st = summary.reference_stats(np.array([1.0, v, 2.0], dtype=np.float32), limits)
        assert st["n_nonfinite"] == 1 and st["counts"].sum() == 2
        with pytest.raises(ValueError, match="Nan in summary histogram for: SCORE/cls_score/scores"):
            summary.histogram("SCORE/cls_score/scores", st, limits)


def test_ground_truth_picture_is_drawn_at_the_original_scale():
    from utils.visualization import draw_bounding_boxes, resize_bilinear
    img = np.full((60, 100, 3), 200.0, dtype=np.float32)
    small = resize_bilinear(img, 30, 50)
    assert small.shape == (30, 50, 3) and np.all(small == 200.0)
    out = draw_bounding_boxes(small, np.array([[20, 20, 80, 50, 3]], dtype=np.float32), (60.0, 100.0, 2.0))
    assert out.shape == (1, 30, 50, 3) and out.dtype == np.float32
    changed = np.any(out[0] != 200.0, axis=2)
    ys, xs = np.where(changed)
    assert changed.any() and xs.min() == 10 and ys.max() == 25           # the box edges at gt / im_scale
