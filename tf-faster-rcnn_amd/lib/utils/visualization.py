"""utils.visualization -- host mirror of the reference's lib/utils/visualization.py:71-89 (draw_bounding_boxes, the py_func behind the
GROUND_TRUTH image summary, lib/nets/network.py:40-55): the ground-truth boxes drawn on the image at its ORIGINAL scale, one colour per
class, labelled "N<box index>-C<class>", PIL's default bitmap font.  Host code, run once per summary interval."""
import numpy as np
from PIL import Image, ImageDraw, ImageFont

# a fixed palette in the spirit of the reference's colour-name list (any distinguishable set does: the picture is for a person)
COLORS = [(230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180), (70, 240, 240), (240, 50, 230),
          (210, 245, 60), (250, 190, 190), (0, 128, 128), (230, 190, 255), (170, 110, 40), (255, 250, 200), (128, 0, 0), (170, 255, 195),
          (128, 128, 0), (255, 215, 180), (0, 0, 128), (128, 128, 128), (255, 255, 255)]


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
