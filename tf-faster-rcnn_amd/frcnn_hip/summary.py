"""TensorBoard event files without TensorFlow: what the reference gets from tf.summary.* and tf.summary.FileWriter
(lib/nets/network.py:47-66,437-450, lib/model/train_val.py:149-151,281-290).

Messages (tensorflow/core/util/event.proto, core/framework/summary.proto), encoded with the wire helpers of tensor_bundle.py:

  Event          wall_time 1 (double), step 2 (int64), file_version 3 (string, "brain.Event:2"), summary 5 (Summary)
  Summary        value 1 (repeated Value)
  Summary.Value  tag 1, simple_value 2 (float), image 4 (Summary.Image), histo 5 (HistogramProto)
  Summary.Image  height 1, width 2, colorspace 3, encoded_image_string 4 (PNG, written by PIL)
  HistogramProto min 1, max 2, num 3, sum 4, sum_squares 5 (doubles), bucket_limit 6, bucket 7 (packed doubles)

An event file is a TFRecord file (core/lib/io/record_writer.cc): per record u64 length, masked crc32c of those 8 bytes, payload, masked
crc32c of the payload (all little endian); the first record is the version event.  File name: events.out.tfevents.<secs>.<host>.

Histograms: the statistics come from ops.summary_stats (csrc/summary_stats.hip) over TensorFlow's 1551 default buckets; `compress_buckets`
writes them as tensorflow/core/lib/histogram/histogram.cc Histogram::EncodeToProto does -- every run of empty buckets collapsed into one
entry that carries the run's LAST limit.  PARITY UNPINNED: that rule is restated from the TensorFlow r1.2 source as remembered; neither
TensorFlow nor TensorBoard exists here to compare bytes with.  TensorBoard reads any increasing limit list.
A tensor with a NaN or an infinity raises ValueError("Nan in summary histogram for: <tag>") like tf.summary.histogram's kernel."""
import io
import os
import socket
import struct
import time

import numpy as np

from .tensor_bundle import _pb_bytes, _pb_varint, _put_varint, crc32c, mask_crc

FILE_VERSION = "brain.Event:2"


# ------------------------------------------------------------------------------------------------ protobuf wire
def _pb_double(field, v):
    return _put_varint((field << 3) | 1) + struct.pack("<d", float(v))


def _pb_float(field, v):
    return _put_varint((field << 3) | 5) + struct.pack("<f", float(v))


def _pb_packed_doubles(field, values):
    return _pb_bytes(field, np.ascontiguousarray(values, dtype="<f8").tobytes())


# ------------------------------------------------------------------------------------------------ Summary values
def scalar(tag, value):
    """One serialised Summary.Value entry of a Summary (tf.summary.scalar)."""
    return _pb_bytes(1, _pb_bytes(1, tag.encode()) + _pb_float(2, value))


def compress_buckets(counts, limits):
    """Dense counts over `limits` -> (bucket_limit, bucket) as Histogram::EncodeToProto writes them: an entry per non-empty bucket, and
    ONE entry (the run's last limit, count 0) per run of empty buckets; an all-empty histogram is the single entry (DBL_MAX, 0)."""
    counts = np.asarray(counts)
    if counts.size == 0:
        return [float(np.finfo(np.float64).max)], [0.0]
    filled = counts > 0
    # an empty bucket is written only as the LAST of its run: the one before a filled bucket, or the table's last
    keep = filled | np.append(filled[1:], True)
    return np.asarray(limits, dtype=np.float64)[keep].tolist(), np.where(filled, counts, 0)[keep].astype(np.float64).tolist()


def histogram(tag, stats, limits):
    """One serialised Summary.Value (tf.summary.histogram) from a record of ops.summary_stats / reference_stats."""
    if stats["n_nonfinite"] > 0:
        raise ValueError("Nan in summary histogram for: %s" % tag)
    lim, cnt = compress_buckets(stats["counts"], limits)
    h = (_pb_double(1, stats["min"]) + _pb_double(2, stats["max"]) + _pb_double(3, stats["num"]) + _pb_double(4, stats["sum"])
         + _pb_double(5, stats["sum_squares"]) + _pb_packed_doubles(6, lim) + _pb_packed_doubles(7, cnt))
    return _pb_bytes(1, _pb_bytes(1, tag.encode()) + _pb_bytes(5, h))


def zero_fraction(stats):
    """tf.nn.zero_fraction of the summarised tensor: the share of x == 0 among ALL elements."""
    return float(stats["n_zero"]) / float(stats["num"]) if stats["num"] else 0.0


def image(tag, rgb):
    """One serialised Summary.Value (tf.summary.image, one image): rgb uint8 [H,W,3] -> PNG; the tag gets tf's "/image/0" suffix."""
    from PIL import Image
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="PNG", compress_level=1)          # (fast setting: one picture per summary, read once)
    img = _pb_varint(1, rgb.shape[0]) + _pb_varint(2, rgb.shape[1]) + _pb_varint(3, rgb.shape[2]) + _pb_bytes(4, buf.getvalue())
    return _pb_bytes(1, _pb_bytes(1, (tag + "/image/0").encode()) + _pb_bytes(4, img))


def event(wall_time, step, summary=None, file_version=None):
    out = _pb_double(1, wall_time)
    if step:
        out += _pb_varint(2, int(step))
    if file_version is not None:
        out += _pb_bytes(3, file_version.encode())
    if summary is not None:
        out += _pb_bytes(5, bytes(summary))
    return out


def record(payload):
    """One TFRecord: length, masked crc of the length, payload, masked crc of the payload."""
    head = struct.pack("<Q", len(payload))
    return head + struct.pack("<I", mask_crc(crc32c(head))) + payload + struct.pack("<I", mask_crc(crc32c(payload)))


class FileWriter(object):
    """tf.summary.FileWriter(logdir): appends events to <logdir>/events.out.tfevents.<secs>.<host>; the version record is written when
    the file is opened."""

    def __init__(self, logdir):
        os.makedirs(logdir, exist_ok=True)
        now = time.time()
        self.path = os.path.join(logdir, "events.out.tfevents.%010d.%s" % (int(now), socket.gethostname()))
        self._f = open(self.path, "ab")
        self._f.write(record(event(now, 0, file_version=FILE_VERSION)))
        self._f.flush()

    def add_summary(self, summary, global_step=None):
        """summary: a serialised Summary (bytes), as Network.train_step_with_summary / get_summary return it"""
        self._f.write(record(event(time.time(), int(global_step or 0), summary=summary)))

    def flush(self):
        self._f.flush()

    def close(self):
        if not self._f.closed:
            self._f.flush()
            self._f.close()


# ------------------------------------------------------------------------------------------------ numpy statement of the statistics
def reference_stats(x, limits):
    """Second statement of ops.summary_stats for one tensor, on the host: np.searchsorted(side='right') is upper_bound, math.fsum the
    exactly rounded sums; limits = ops.summary_limits().  Same record, same conventions (a non-finite value is counted in n_nonfinite only; min / max of no value are
    DBL_MAX / -DBL_MAX)."""
    import math
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    fin = np.isfinite(x)
    d = x[fin].astype(np.float64)
    counts = np.bincount(np.searchsorted(limits, d, side="right"), minlength=len(limits)).astype(np.int64)
    big = float(np.finfo(np.float64).max)
    return dict(counts=counts, num=int(x.size), n_zero=int(np.count_nonzero(d == 0.0)), n_nonfinite=int(x.size - d.size),
                min=float(d.min()) if d.size else big, max=float(d.max()) if d.size else -big,
                sum=math.fsum(d.tolist()), sum_squares=math.fsum((d * d).tolist()))
