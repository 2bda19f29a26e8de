"""roi_data_layer.minibatch -- one training minibatch from one roidb entry (lib/roi_data_layer/minibatch.py:19-74).

The reference decodes, mirrors, mean-subtracts and resizes the image on the host (cv2) and returns the float `data` blob.  Here the
resize is a device kernel (frcnn_prep_train_image), so the blob carries the RAW image instead -- `image` uint8 BGR [h,w,3] as decoded (numpy; a device tensor under
cfg.HIP.JPEG_DEVICE), `flipped`, `target_size`, `max_size` -- plus the roidb's `boxes` uint16 / `gt_classes` int32 rows the kernel turns into the device gt
buffer.  `im_info` and `gt_boxes` are the reference's arrays (nets.network stages the blob: Network._stage_train_inputs)."""
import numpy as np
import numpy.random as npr

from model.config import cfg


def read_image(path):
    """BGR uint8 [h,w,3] like cv2.imread, decoded with PIL (model.test.imdb_images)."""
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(path).convert("RGB"))[:, :, ::-1])


def draw_scales(num_images):
    """minibatch.py:23-24: the one draw a minibatch takes from the global numpy stream."""
    return npr.randint(0, high=len(cfg.TRAIN.SCALES), size=num_images)


def read_image_device(path):
    """cfg.HIP.JPEG_DEVICE: the same pixels as a uint8 device tensor (frcnn_hip.jpeg: host Huffman stage, IDCT + colour kernels)."""
    import torch
    from frcnn_hip.jpeg import decode_bgr
    return decode_bgr(path, torch.device("cuda", torch.cuda.current_device()))


def get_minibatch(roidb, num_classes, scale_inds=None, image=None):
    """image: the entry's decoded image when the caller already has it (RoIDataLayer's prefetch under cfg.HIP.JPEG_DEVICE)."""
    from frcnn_hip import ops
    num_images = len(roidb)
    if scale_inds is None:
        scale_inds = draw_scales(num_images)
    assert cfg.TRAIN.BATCH_SIZE % num_images == 0, 'num_images ({}) must divide BATCH_SIZE ({})'.format(num_images, cfg.TRAIN.BATCH_SIZE)
    assert num_images == 1, "Single batch only"
    entry = roidb[0]
    if image is not None:
        im = image
    else:
        im = read_image_device(entry['image']) if cfg.HIP.JPEG_DEVICE else read_image(entry['image'])
    target_size = int(cfg.TRAIN.SCALES[scale_inds[0]])
    im_scale, OH, OW = ops.prep_image_shape(im.shape[0], im.shape[1], target_size, cfg.TRAIN.MAX_SIZE)      # blob.py:37-45
    # minibatch.py:38-43: USE_ALL_GT or not, the reference's expression selects gt_classes != 0 (`0 & ...` binds first in the crowd branch)
    gt_inds = np.where(entry['gt_classes'] != 0)[0]
    boxes = np.ascontiguousarray(entry['boxes'][gt_inds, :])
    classes = np.ascontiguousarray(entry['gt_classes'][gt_inds])
    gt_boxes = np.empty((len(gt_inds), 5), dtype=np.float32)
    gt_boxes[:, 0:4] = boxes * im_scale                          # uint16 * Python float -> float64, rounded once on assignment
    gt_boxes[:, 4] = classes
    return {'image': im, 'flipped': bool(entry['flipped']), 'target_size': target_size, 'max_size': int(cfg.TRAIN.MAX_SIZE),
            'boxes': boxes, 'gt_classes': classes, 'gt_boxes': gt_boxes,
            'im_info': np.array([OH, OW, im_scale], dtype=np.float32)}
