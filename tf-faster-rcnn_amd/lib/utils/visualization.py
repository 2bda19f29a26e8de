"""utils.visualization -- host mirror of the reference's lib/utils/visualization.py:71-89 (draw_bounding_boxes, the py_func behind the
GROUND_TRUTH image summary, lib/nets/network.py:40-55): the ground-truth boxes drawn on the image at its ORIGINAL scale, one colour per
class, labelled "N<box index>-C<class>", PIL's default bitmap font.  Host code, run once per summary interval.

draw_detections is the device counterpart for tools/demo.py: detection records and their device-resident count drawn in place by one
launch (frcnn_draw_detections), with this module's own 5 x 7 font, class names and colours as its tables."""
import numpy as np
from PIL import Image, ImageDraw, ImageFont

# a fixed palette in the spirit of the reference's colour-name list (any distinguishable set does: the picture is for a person)
COLORS = [(230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180), (70, 240, 240), (240, 50, 230),
          (210, 245, 60), (250, 190, 190), (0, 128, 128), (230, 190, 255), (170, 110, 40), (255, 250, 200), (128, 0, 0), (170, 255, 195),
          (128, 128, 0), (255, 215, 180), (0, 0, 128), (128, 128, 128), (255, 255, 255)]


# The 5 x 7 bitmap font of draw_detections, this project's own: printable ASCII in order, seven rows per glyph, a row's bit 4 is its left
# column (0x1F = a full row).  Lower-case letters sit on rows 2..6, descenders use rows 1..6.
FONT_5X7 = {
    " ": "00 00 00 00 00 00 00", "!": "04 04 04 04 00 00 04", '"': "0A 0A 0A 00 00 00 00", "#": "0A 0A 1F 0A 1F 0A 0A",
    "$": "04 0F 14 0E 05 1E 04", "%": "18 19 02 04 08 13 03", "&": "0C 12 14 08 15 12 0D", "'": "0C 04 08 00 00 00 00",
    "(": "02 04 08 08 08 04 02", ")": "08 04 02 02 02 04 08", "*": "00 04 15 0E 15 04 00", "+": "00 04 04 1F 04 04 00",
    ",": "00 00 00 00 0C 04 08", "-": "00 00 00 1F 00 00 00", ".": "00 00 00 00 00 0C 0C", "/": "00 01 02 04 08 10 00",
    "0": "0E 11 13 15 19 11 0E", "1": "04 0C 04 04 04 04 0E", "2": "0E 11 01 02 04 08 1F", "3": "1F 02 04 02 01 11 0E",
    "4": "02 06 0A 12 1F 02 02", "5": "1F 10 1E 01 01 11 0E", "6": "06 08 10 1E 11 11 0E", "7": "1F 01 02 04 08 08 08",
    "8": "0E 11 11 0E 11 11 0E", "9": "0E 11 11 0F 01 02 0C", ":": "00 0C 0C 00 0C 0C 00", ";": "00 0C 0C 00 0C 04 08",
    "<": "02 04 08 10 08 04 02", "=": "00 00 1F 00 1F 00 00", ">": "08 04 02 01 02 04 08", "?": "0E 11 01 02 04 00 04",
    "@": "0E 11 01 0D 15 15 0E", "A": "0E 11 11 1F 11 11 11", "B": "1E 11 11 1E 11 11 1E", "C": "0E 11 10 10 10 11 0E",
    "D": "1C 12 11 11 11 12 1C", "E": "1F 10 10 1E 10 10 1F", "F": "1F 10 10 1E 10 10 10", "G": "0E 11 10 17 11 11 0F",
    "H": "11 11 11 1F 11 11 11", "I": "0E 04 04 04 04 04 0E", "J": "07 02 02 02 02 12 0C", "K": "11 12 14 18 14 12 11",
    "L": "10 10 10 10 10 10 1F", "M": "11 1B 15 15 11 11 11", "N": "11 11 19 15 13 11 11", "O": "0E 11 11 11 11 11 0E",
    "P": "1E 11 11 1E 10 10 10", "Q": "0E 11 11 11 15 12 0D", "R": "1E 11 11 1E 14 12 11", "S": "0F 10 10 0E 01 01 1E",
    "T": "1F 04 04 04 04 04 04", "U": "11 11 11 11 11 11 0E", "V": "11 11 11 11 11 0A 04", "W": "11 11 11 15 15 15 0A",
    "X": "11 11 0A 04 0A 11 11", "Y": "11 11 11 0A 04 04 04", "Z": "1F 01 02 04 08 10 1F", "[": "0E 08 08 08 08 08 0E",
    "\\": "00 10 08 04 02 01 00", "]": "0E 02 02 02 02 02 0E", "^": "04 0A 11 00 00 00 00", "_": "00 00 00 00 00 00 1F",
    "`": "08 04 02 00 00 00 00", "a": "00 00 0E 01 0F 11 0F", "b": "10 10 16 19 11 11 1E", "c": "00 00 0E 10 10 11 0E",
    "d": "01 01 0D 13 11 11 0F", "e": "00 00 0E 11 1F 10 0E", "f": "06 09 08 1C 08 08 08", "g": "00 0F 11 11 0F 01 0E",
    "h": "10 10 16 19 11 11 11", "i": "04 00 0C 04 04 04 0E", "j": "02 00 06 02 02 12 0C", "k": "10 10 12 14 18 14 12",
    "l": "0C 04 04 04 04 04 0E", "m": "00 00 1A 15 15 11 11", "n": "00 00 16 19 11 11 11", "o": "00 00 0E 11 11 11 0E",
    "p": "00 1E 11 11 1E 10 10", "q": "00 0F 11 11 0F 01 01", "r": "00 00 16 19 10 10 10", "s": "00 00 0F 10 0E 01 1E",
    "t": "08 08 1C 08 08 09 06", "u": "00 00 11 11 11 13 0D", "v": "00 00 11 11 11 0A 04", "w": "00 00 11 11 15 15 0A",
    "x": "00 00 11 0A 04 0A 11", "y": "00 11 11 0F 01 11 0E", "z": "00 00 1F 02 04 08 1F", "{": "02 04 04 08 04 04 02",
    "|": "04 04 04 04 04 04 04", "}": "08 04 04 02 04 04 08", "~": "00 00 08 15 02 00 00",
}
LABEL_STRIDE_MAX = 64


def glyph_table():
    """uint8 [95,7]: FONT_5X7 in ASCII order from the space on, what frcnn_draw_detections reads as glyphs"""
    return np.array([[int(v, 16) for v in FONT_5X7[chr(c)].split()] for c in range(32, 127)], dtype=np.uint8)


def label_table(class_names):
    """uint8 [num_classes, stride]: the names NUL-padded (characters outside printable ASCII become '?'), stride <= 64"""
    names = [str(n).encode("ascii", "replace")[:LABEL_STRIDE_MAX - 1] for n in class_names]
    stride = max(len(n) for n in names) + 1
    out = np.zeros((len(names), stride), dtype=np.uint8)
    for i, n in enumerate(names):
        out[i, :len(n)] = np.frombuffer(n, dtype=np.uint8)
    return out


def colour_table():
    """uint8 [len(COLORS),3]: COLORS stored BGR, like the image"""
    return np.ascontiguousarray(np.array(COLORS, dtype=np.uint8)[:, ::-1])


_tables = {}


def draw_tables(class_names, device):
    """(colours, labels, glyphs) as uint8 tensors on `device`, uploaded once per (class list, device)"""
    import torch
    key = (tuple(class_names), str(device))
    if key not in _tables:
        _tables[key] = tuple(torch.from_numpy(t).to(device) for t in (colour_table(), label_table(class_names), glyph_table()))
    return _tables[key]


def draw_detections(im, dets, cnt, class_names, conf=0.8, thickness=2, scale=1):
    """Detection records drawn on the BGR uint8 image [h,w,3] IN PLACE (include/frcnn_hip.h frcnn_draw_detections states the rule): an
    outline in the class colour and a label plate "<class name> d.ddd" for every record k < min(cnt, len(dets)) with score >= conf.
    Device tensors (im, dets [n,6] and the count [1] int32 exactly as Network.detect_device leaves them): one launch on the current stream,
    nothing is read back.  A numpy image: the host statement of the same rule (dets numpy or CPU tensor, cnt an int or a CPU tensor)."""
    import torch
    from frcnn_hip import ops
    if torch.is_tensor(im) and im.is_cuda:
        return ops.draw_detections(im, dets, cnt, conf, thickness, scale, *draw_tables(class_names, im.device))
    a = im.numpy() if torch.is_tensor(im) else im
    d = dets.numpy() if torch.is_tensor(dets) else np.asarray(dets, dtype=np.float32)
    n = int(cnt.reshape(-1)[0]) if (torch.is_tensor(cnt) or isinstance(cnt, np.ndarray)) else int(cnt)
    ops.draw_detections_host(a, d, n, conf, thickness, scale, *draw_tables(class_names, "cpu"))
    return im


def draw_bounding_boxes(image, gt_boxes, im_info, thickness=4):
    """image: [1,H,W,3] or [H,W,3], RGB, 0..255, ALREADY at the original scale (network.py:44 resizes by 1 / im_info[2] before the
    py_func); gt_boxes [G,5] (x1, y1, x2, y2, class) at the NETWORK's scale -> divided by im_info[2] and rounded (visualization.py:74).
    Returns float32 [1,H,W,3] like the reference's py_func."""
    arr = np.asarray(image)
    arr = arr[0] if arr.ndim == 4 else arr
    pic = Image.fromarray(np.clip(np.rint(arr), 0, 255).astype(np.uint8))
    boxes = np.array(gt_boxes, dtype=np.float64).reshape(-1, 5)
    boxes[:, :4] = np.round(boxes[:, :4] / float(im_info[2]))
    draw = ImageDraw.Draw(pic)
    font = ImageFont.load_default()
    for i, (x1, y1, x2, y2, c) in enumerate(boxes):
        color = COLORS[int(c) % len(COLORS)]
        draw.rectangle([x1, y1, max(x1, x2), max(y1, y2)], outline=color, width=int(thickness))
        label = "N%02d-C%02d" % (i, int(c))
        l, t, r, b = draw.textbbox((0, 0), label, font=font)
        tw, th = r - l, b - t
        ty = y1 - th - 4 if y1 - th - 4 >= 0 else y1                    # above the box, inside it at the top edge of the picture
        draw.rectangle([x1, ty, x1 + tw + 4, ty + th + 4], fill=color)
        draw.text((x1 + 2, ty + 2 - t), label, fill=(0, 0, 0), font=font)
    return np.asarray(pic, dtype=np.float32)[None]


def resize_bilinear(rgb, height, width):
    """tf.image.resize_bilinear's role in network.py:44: the staged image back at its original size (PIL's bilinear filter; the picture is
    for a person, not compared with TensorFlow's sampling)."""
    pic = Image.fromarray(np.clip(np.rint(np.asarray(rgb)), 0, 255).astype(np.uint8))
    if pic.size != (int(width), int(height)):
        pic = pic.resize((int(width), int(height)), Image.BILINEAR)
    return np.asarray(pic, dtype=np.float32)
