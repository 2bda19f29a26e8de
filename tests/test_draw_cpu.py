"""CPU: the host statement of the drawing rule (csrc/draw_math.h, the header the kernel of csrc/draw.hip compiles too) against a numpy
painter written here from the rule's text (include/frcnn_hip.h, frcnn_draw_detections), bit for bit: clipping at the four borders, the label
plate above the box or inside it, the order of overlapping records, the threshold, and the records that must be skipped without a read out
of bounds."""
import numpy as np
import pytest
import torch

import frcnn_hip
from frcnn_hip import ops
from utils import visualization as vis

NAMES = ('__background__', 'aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair', 'cow', 'diningtable', 'dog',
         'horse', 'motorbike', 'person', 'pottedplant', 'sheep', 'sofa', 'train', 'tvmonitor')
SHAPES = [(64, 96), (97, 523)]
CONF = 0.8
NAN = float("nan")


def image(h, w):
    return np.random.RandomState(h * 1000 + w).randint(0, 256, (h, w, 3)).astype(np.uint8)


def records(h, w):
    """(dets float32 [24,6], cnt): the 20 records below, then rows beyond cnt filled with NaN"""
    rows = [
        (w * 0.30, h * 0.40, w * 0.62, h * 0.81, 0.93, 7),            # interior
        (-9.6, h * 0.30, w * 0.21, h * 0.55, 0.88, 12),              # clipped at the left border, negative coordinate
        (w * 0.80, h * 0.35, w + 14.2, h * 0.62, 0.91, 3),           # right border, coordinate past the edge (the plate is clipped too)
        (w * 0.40, -7.5, w * 0.70, h * 0.20, 0.97, 15),              # top border: the plate goes inside the box
        (w * 0.10, h * 0.70, w * 0.45, h + 9.0, 0.85, 19),           # bottom border
        (w * 0.55, 3.2, w * 0.78, h * 0.33, 0.99, 1),                # too close to the top edge for a plate above: inside
        (w * 0.35, h * 0.45, w * 0.70, h * 0.90, 0.89, 9),           # overlaps the first record: painted over it ...
        (w * 0.33, h * 0.50, w * 0.50, h * 0.75, 0.90, 20),          # ... and this one over both
        (w * 0.05, h * 0.20, w * 0.05 + 2.0, h * 0.20 + 40.0, 0.95, 5),          # thickness greater than half the box: all outline
        (w * 0.60, h * 0.60, w * 0.90, h * 0.95, np.nextafter(np.float32(CONF), np.float32(0)), 2),      # just below conf: not drawn
        (w * 0.62, h * 0.10, w * 0.95, h * 0.30, np.float32(CONF), 4),                                  # equal to conf: drawn
        (w * 0.50, h * 0.50, w * 0.50 - 1.0, h * 0.80, 0.99, 6),     # degenerate: x2 < x1 after rounding
        (NAN, h * 0.10, w * 0.30, h * 0.30, 0.99, 8),                # a NaN coordinate
        (w * 0.10, h * 0.10, w * 0.30, NAN, 0.99, 8),
        (w * 0.10, h * 0.10, w * 0.30, h * 0.30, 0.99, 21),          # classes outside the table
        (w * 0.10, h * 0.10, w * 0.30, h * 0.30, 0.99, -1),
        (w * 0.10, h * 0.10, w * 0.30, h * 0.30, NAN, 3),            # a NaN score
        (w + 5.0, h * 0.10, w + 40.0, h * 0.30, 0.99, 3),            # wholly outside the picture
        (2.5, h * 0.55, 20.5, h * 0.66, np.float32(0.9995), 10),     # halves round to even: 2, 20; the score prints as 1.000
        (w * 0.70, h * 0.70, w * 0.70, h * 0.70, 0.9994, 11),        # a single pixel; prints as 0.999
        (1e9, 0.0, 2e9, 10.0, 0.99, 3),                              # far outside: skipped, never converted to an int
    ]
    dets = np.full((24, 6), NAN, dtype=np.float32)
    dets[:len(rows)] = np.array(rows, dtype=np.float32)
    return dets, len(rows)


def thousandths(score):
    """m of the rule: min(1000, (int)(score * 1000.0f + 0.5f)), every operation in float32"""
    return min(1000, int(np.float32(np.float32(score) * np.float32(1000.0)) + np.float32(0.5)))


def label_of(name, score):
    m = thousandths(score)
    return "%s %d.%03d" % (name, m // 1000, m % 1000)


def paint(im, dets, cnt, conf=CONF, thickness=2, scale=1, names=NAMES):
    """the rule, restated with numpy slices; in place"""
    h, w = im.shape[:2]
    glyphs, pad = vis.glyph_table(), 2
    for k in range(min(int(cnt), len(dets))):
        box, score, cls = dets[k, :4], dets[k, 4], dets[k, 5]
        if not np.all(np.abs(box) <= 2.0 ** 20):                     # NaN compares false
            continue
        if not score >= np.float32(conf) or not (0 <= cls < len(names)):
            continue
        X1, Y1, X2, Y2 = [int(v) for v in np.rint(box)]              # float32 round-half-even, rintf
        if X2 < X1 or Y2 < Y1:
            continue
        X1, Y1, X2, Y2 = max(X1, 0), max(Y1, 0), min(X2, w - 1), min(Y2, h - 1)
        if X2 < X1 or Y2 < Y1:
            continue
        c = int(cls)
        colour = np.array(vis.COLORS[c % len(vis.COLORS)][::-1], dtype=np.uint8)
        ring = np.ones((Y2 - Y1 + 1, X2 - X1 + 1), dtype=bool)
        if X2 - thickness >= X1 + thickness and Y2 - thickness >= Y1 + thickness:
            ring[thickness:ring.shape[0] - thickness, thickness:ring.shape[1] - thickness] = False
        im[Y1:Y2 + 1, X1:X2 + 1][ring] = colour
        text = label_of(names[c], score)
        ph, pw = 7 * scale + 2 * pad, len(text) * 6 * scale + 2 * pad
        plate = np.empty((ph, pw, 3), dtype=np.uint8)
        plate[:] = colour
        for i, ch in enumerate(text):
            bits = (glyphs[ord(ch) - 32][:, None] >> (4 - np.arange(5))[None, :]) & 1          # [7,5]
            ink = np.kron(bits, np.ones((scale, scale), dtype=np.uint8)).astype(bool)
            cell = plate[pad:pad + 7 * scale, pad + i * 6 * scale:pad + i * 6 * scale + 5 * scale]
            cell[ink] = 0
        py0 = Y1 - ph if Y1 - ph >= 0 else Y1
        part = plate[:min(h, py0 + ph) - py0, :min(w, X1 + pw) - X1]
        im[py0:py0 + part.shape[0], X1:X1 + part.shape[1]] = part
    return im


def host(im, dets, cnt, conf=CONF, thickness=2, scale=1, names=NAMES):
    return vis.draw_detections(im, dets, cnt, names, conf=conf, thickness=thickness, scale=scale)


def test_the_font_covers_printable_ascii():
    g = vis.glyph_table()
    assert g.shape == (95, 7) and g.dtype == np.uint8 and int(g.max()) < 32
    assert not g[0].any() and all(g[i].any() for i in range(1, 95))                  # the space is blank, nothing else is
    assert len({bytes(r) for r in g}) == 95                                          # no two glyphs alike
    lab = vis.label_table(NAMES)
    assert lab.shape == (21, 15) and bytes(lab[11]).rstrip(b"\0") == b"diningtable" and not lab[:, -1].any()
    assert np.array_equal(vis.colour_table()[0], np.array(vis.COLORS[0][::-1], dtype=np.uint8))


def test_scores_print_by_the_float32_rule():
    """0.9995 and 0.99949997 are the same float32 (0.999499976...): times 1000.0f it rounds to 999.5, plus 0.5f is 1000 -> "1.000", where
    decimal arithmetic would print 0.999"""
    assert np.float32(0.9995) == np.float32(0.99949997)
    assert thousandths(0.9995) == thousandths(0.99949997) == 1000 and label_of("cow", 0.9995) == "cow 1.000"
    assert thousandths(np.nextafter(np.float32(0.9995), np.float32(0))) == 999
    assert thousandths(0.9994) == 999 and thousandths(0.8) == 800 and thousandths(1.0) == 1000 and label_of("cat", 0.80449) == "cat 0.804"
    for score in (0.9995, 0.99949997, float(np.nextafter(np.float32(0.9995), np.float32(0))), 0.8005):
        dets = np.array([[10, 30, 80, 50, score, 8]], dtype=np.float32)
        for scale in (1, 2):
            base = image(64, 96)
            assert np.array_equal(host(base.copy(), dets, 1, scale=scale), paint(base.copy(), dets, 1, scale=scale)), (score, scale)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("thickness,scale", [(2, 1), (1, 2), (5, 3)])
def test_host_draw_equals_the_numpy_painter(shape, thickness, scale):
    h, w = shape
    base = image(h, w)
    dets, cnt = records(h, w)
    want = paint(base.copy(), dets, cnt, thickness=thickness, scale=scale)
    got = host(base.copy(), dets, cnt, thickness=thickness, scale=scale)
    assert np.array_equal(got, want)
    changed = (want != base).any(axis=2)
    assert 0.05 < changed.mean() < 0.9                                               # something was drawn, not everything
    # every record alone, and every prefix: the order of overlapping records is part of the picture
    for k in range(cnt):
        one = np.full((3, 6), NAN, dtype=np.float32)
        one[0] = dets[k]
        assert np.array_equal(host(base.copy(), one, 1, thickness=thickness, scale=scale), paint(base.copy(), one, 1, thickness=thickness, scale=scale)), k
    assert np.array_equal(host(base.copy(), dets, 8, thickness=thickness, scale=scale), paint(base.copy(), dets, 8, thickness=thickness, scale=scale))
    swapped = dets.copy()
    swapped[[0, 7]] = dets[[7, 0]]
    a = host(base.copy(), swapped, cnt, thickness=thickness, scale=scale)
    assert np.array_equal(a, paint(base.copy(), swapped, cnt, thickness=thickness, scale=scale)) and not np.array_equal(a, want)


def test_skipped_records_and_an_empty_count_leave_the_image_untouched():
    h, w = SHAPES[0]
    base = image(h, w)
    dets, cnt = records(h, w)
    assert np.array_equal(host(base.copy(), dets, 0), base)                           # cnt = 0
    assert np.array_equal(host(base.copy(), dets, -3), base)
    skipped = dets[[9, 11, 12, 13, 14, 15, 16, 17, 20, 21, 22, 23]]                   # below conf, degenerate, NaN, bad class, outside, beyond cnt
    assert np.array_equal(host(base.copy(), skipped, len(skipped)), base)
    assert np.array_equal(paint(base.copy(), skipped, len(skipped)), base)
    # a count beyond the record is capped at max_dets: the NaN rows behind cnt draw nothing, nothing behind the array is read
    assert np.array_equal(host(base.copy(), dets, 10 ** 6), paint(base.copy(), dets, cnt))
    # the box whose score equals conf is drawn, the one just below is not
    assert not np.array_equal(host(base.copy(), dets[10:11], 1), base) and np.array_equal(host(base.copy(), dets[9:10], 1), base)


def test_arguments_outside_the_rule_are_refused():
    lib = frcnn_hip.lib()
    im = image(8, 8)
    dets = np.zeros((1, 6), dtype=np.float32)
    col, lab, gly = (torch.from_numpy(t) for t in (vis.colour_table(), vis.label_table(NAMES), vis.glyph_table()))

    def rc(h=8, w=8, thickness=2, scale=1, ncol=21, ncls=21, stride=15, glyphs=gly.data_ptr()):
        return lib.frcnn_draw_detections_host(im.ctypes.data, h, w, dets.ctypes.data, 1, 1, 0.5, thickness, scale, col.data_ptr(), ncol,
                                              lab.data_ptr(), ncls, stride, glyphs)
    assert rc() == 0
    for bad in (dict(h=0), dict(w=0), dict(thickness=0), dict(scale=0), dict(scale=17), dict(ncol=0), dict(ncls=0), dict(stride=0),
                dict(stride=65), dict(glyphs=None)):
        assert rc(**bad) == -1, bad
    from frcnn_hip import replay
    assert {"frcnn_draw_detections", "frcnn_draw_detections_host"} <= set(frcnn_hip.SIGNATURES)
    assert "frcnn_draw_detections_host" in replay.HOST_ONLY and "frcnn_draw_detections" not in replay.HOST_ONLY
