"""roi_data_layer.layer -- the training data layer of the reference (lib/roi_data_layer/layer.py:21-88).

RoIDataLayer walks a permutation of the roidb and consumes the GLOBAL numpy random stream exactly like the reference: one permutation per
shuffle (three with cfg.TRAIN.ASPECT_GROUPING, which needs an even roidb length), a reshuffle when `cur + IMS_PER_BATCH >= len` (so the
last entry of a permutation is never served), one randint per minibatch for the scale.  With np.random seeded the same, the sequence of
(roidb index, scale) equals the reference's.

Data parallel (no counterpart in the reference): every rank runs the SAME stream -- same seed, same roidb -- and rank r of W trains on
minibatches r, r+W, ... of it; the others are drawn (indices and scale, no image decode) and skipped.  W = 1 is the reference sequence."""
import time

import numpy as np

from model.config import cfg
from roi_data_layer.minibatch import draw_scales, get_minibatch


class RoIDataLayer(object):
    def __init__(self, roidb, num_classes, random=False, rank=0, world_size=1):
        assert 0 <= rank < world_size
        self._roidb = roidb
        self._num_classes = num_classes
        self._random = random                        # shuffle by wall clock without touching the global stream (validation sets)
        self._rank, self._world_size = int(rank), int(world_size)
        self._count = 0                              # minibatches drawn from the stream so far, whichever rank they belong to
        self.last_draw = None                        # (roidb index, scale index) of the minibatch forward() returned last
        self._jpeg = None                            # cfg.HIP.JPEG_DEVICE: a frcnn_hip.jpeg.JpegCache decoding the next entries ahead
        self._shuffle_roidb_inds()

    def _shuffle_roidb_inds(self):
        if self._random:
            st0 = np.random.get_state()
            np.random.seed(int(round(time.time() * 1000)) % 4294967295)
        if cfg.TRAIN.ASPECT_GROUPING:
            widths = np.array([r['width'] for r in self._roidb])
            heights = np.array([r['height'] for r in self._roidb])
            horz = widths >= heights
            inds = np.hstack((np.random.permutation(np.where(horz)[0]), np.random.permutation(np.where(~horz)[0])))
            inds = np.reshape(inds, (-1, 2))
            row_perm = np.random.permutation(np.arange(inds.shape[0]))
            self._perm = np.reshape(inds[row_perm, :], (-1,))
        else:
            self._perm = np.random.permutation(np.arange(len(self._roidb)))
        if self._random:
            np.random.set_state(st0)
        self._cur = 0

    def _get_next_minibatch_inds(self):
        if self._cur + cfg.TRAIN.IMS_PER_BATCH >= len(self._roidb):
            self._shuffle_roidb_inds()
        db_inds = self._perm[self._cur:self._cur + cfg.TRAIN.IMS_PER_BATCH]
        self._cur += cfg.TRAIN.IMS_PER_BATCH
        return db_inds

    def _draw(self):
        """The next minibatch of the stream: (roidb indices, scale indices), in the reference's order of draws."""
        db_inds = self._get_next_minibatch_inds()
        scale_inds = draw_scales(len(db_inds))
        self._count += 1
        return db_inds, scale_inds

    def forward(self):
        """Blobs of this rank's next minibatch (roi_data_layer.minibatch.get_minibatch)."""
        while True:
            mine = (self._count % self._world_size) == self._rank
            db_inds, scale_inds = self._draw()
            if mine:
                break
        self.last_draw = (int(db_inds[0]), int(scale_inds[0]))
        return get_minibatch([self._roidb[i] for i in db_inds], self._num_classes, scale_inds,
                             image=self._decoded(db_inds) if cfg.HIP.JPEG_DEVICE else None)

    JPEG_AHEAD = 4                                   # entries of the permutation decoded ahead (host Huffman stage on worker threads)

    def _decoded(self, db_inds):
        """The image of this minibatch as a device tensor, and the Huffman stage of this rank's next entries of the CURRENT permutation
        started on worker threads (peeked: nothing is drawn from the random stream; the entries after a reshuffle are not known yet)."""
        import torch
        from frcnn_hip.jpeg import JpegCache
        if self._jpeg is None:
            self._jpeg = JpegCache(torch.device("cuda", torch.cuda.current_device()), workers=4, depth=2 * self.JPEG_AHEAD)
        path = self._roidb[int(db_inds[0])]['image']
        im = self._jpeg.get(path, path)
        step = cfg.TRAIN.IMS_PER_BATCH
        pos = self._cur + ((self._rank - self._count) % self._world_size) * step
        for _ in range(self.JPEG_AHEAD):
            if pos + step >= len(self._roidb):       # that draw reshuffles first
                break
            nxt = self._roidb[int(self._perm[pos])]['image']
            self._jpeg.prefetch(nxt, nxt)
            pos += self._world_size * step
        return im

    def __iter__(self):
        return self

    def __next__(self):
        return self.forward()

    next = __next__

    # ---- what a snapshot keeps (model.train_val.SolverWrapper.snapshot / restore; train_val.py:57-78, 89-101 of the reference) ----
    def get_state(self):
        return {'cur': int(self._cur), 'perm': np.array(self._perm), 'count': int(self._count)}

    def set_state(self, state):
        self._cur, self._perm = int(state['cur']), np.array(state['perm'])
        self._count = int(state.get('count', 0))
