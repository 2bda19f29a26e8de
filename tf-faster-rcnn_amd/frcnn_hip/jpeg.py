"""frcnn_hip.jpeg -- image files to BGR uint8 [h,w,3] device tensors, the input of frcnn_prep_image / frcnn_prep_train_image.

A baseline JPEG takes the hybrid path: the Huffman stage on the host (frcnn_jpeg_entropy_decode, C, the GIL released), IDCT, chroma
upsampling and colour conversion in two kernels (frcnn_jpeg_pixels).  The pixels equal `PIL.Image.open(f).convert("RGB")[:, :, ::-1]` bit
for bit.  Every other file -- a JPEG outside the decoder's list (progressive, CMYK, ...), a damaged one, a PNG -- goes the way it always
went: PIL on the host, then the copy; the user sees PIL's pixels or PIL's error.

decode_bgr: one file, synchronous.  JpegCache / JpegPrefetcher: worker threads read files and entropy-decode into a pool of pinned
buffers ahead of the consumer, which issues the copy and the two launches on ITS current stream; a pinned buffer is written again only
after an event recorded behind its copy has completed.

The other direction mirrors it: encode_bgr / JpegWriter turn a BGR tensor into a baseline JPEG file -- colour conversion, downsampling, DCT
and quantisation in two kernels (frcnn_jpeg_coefs) into the SAME coefficient buffer, the Huffman stage on the host
(frcnn_jpeg_entropy_encode).  The coefficients equal those of PIL's encoder at the same quality and subsampling bit for bit."""
import io
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import ops

MAX_WORKERS = 8


def _read(src):
    if isinstance(src, (bytes, bytearray, memoryview)):
        return bytes(src)
    with open(src, "rb") as f:
        return f.read()


def pil_bgr(src):
    """The path every image took before: BGR uint8 [h,w,3] numpy, decoded by PIL (path or bytes)."""
    from PIL import Image
    f = io.BytesIO(bytes(src)) if isinstance(src, (bytes, bytearray, memoryview)) else src
    return np.ascontiguousarray(np.asarray(Image.open(f).convert("RGB"))[:, :, ::-1])


def _is_cuda(device):
    return torch.device(device).type == "cuda"


def _into(t, out):
    """t, or `out` holding t's pixels (a caller's slot of a batch buffer; the shapes must agree)"""
    if out is None:
        return t
    out.copy_(t, non_blocking=True)
    return out


def _pixels(coef_d, geom, out):
    """ops.jpeg_pixels into `out` directly where the colour kernel's dword stores allow it (a 4-byte aligned address; slot k of a batch
    buffer starts k * h * w * 3 bytes in, which is not one when h * w is no multiple of 4), else into a tensor of its own and a copy"""
    if out is None or out.data_ptr() % 4 == 0:
        return ops.jpeg_pixels(coef_d, geom, out=out)
    return _into(ops.jpeg_pixels(coef_d, geom), out)


def decode_bgr(src, device, out=None):
    """File path or bytes -> BGR uint8 [h,w,3] tensor on `device`.  device 'cpu': the host statement of the kernels.
    out: a [h,w,3] uint8 tensor on `device` to decode into (the kernels write it directly where its address is 4-byte aligned)."""
    data = _read(src)
    try:
        geom = ops.jpeg_info(data)
        coef = ops.jpeg_entropy_decode(data, geom=geom)
    except ops.JpegError:
        return _into(torch.from_numpy(pil_bgr(src)).to(device), out)
    if not _is_cuda(device):
        return _into(torch.from_numpy(ops.jpeg_pixels_host(coef, geom)), out)
    return _pixels(coef.to(device), geom, out)


class _Slot(object):
    __slots__ = ("buf", "ev")

    def __init__(self):
        self.buf, self.ev = None, None


class JpegCache(object):
    """prefetch(key, src) starts reading + entropy-decoding `src` on a worker thread if one of the `depth` pinned buffers is free;
    get(key, src) returns the device tensor (decoding synchronously what was never prefetched), `out` given: that tensor, written directly."""

    MIN_SLOT_BYTES = 1 << 20         # a 480 x 640 4:2:0 image needs 0.46 MB: most slots are allocated once

    def __init__(self, device, workers=4, depth=8):
        self.device = torch.device(device)
        self._cuda = _is_cuda(device)
        self._pool = ThreadPoolExecutor(max_workers=max(1, min(int(workers), MAX_WORKERS)))
        self._slots = [_Slot() for _ in range(max(1, int(depth)))]
        self._free = list(range(len(self._slots)))
        self._pending = {}           # key -> (future, slot index)

    def _work(self, src, k):
        data = _read(src)
        try:
            geom = ops.jpeg_info(data)
        except ops.JpegError:
            return ("pil", pil_bgr(src))
        slot = self._slots[k]
        if slot.ev is not None:
            slot.ev.synchronize()                                # the copy that last read this buffer has finished
        n = ops.jpeg_coef_bytes(geom)
        if slot.buf is None or slot.buf.numel() < n:
            slot.buf = torch.empty(max(n, self.MIN_SLOT_BYTES), dtype=torch.uint8, pin_memory=self._cuda)
        try:
            coef = ops.jpeg_entropy_decode(data, out=slot.buf, geom=geom)
        except ops.JpegError:
            return ("pil", pil_bgr(src))
        return ("coef", geom, coef)

    def prefetch(self, key, src):
        if key in self._pending:
            return True
        if not self._free:
            return False
        k = self._free.pop()
        self._pending[key] = (self._pool.submit(self._work, src, k), k)
        return True

    def get(self, key, src, out=None):
        if key not in self._pending:
            return decode_bgr(src, self.device, out)
        fut, k = self._pending.pop(key)
        try:
            res = fut.result()
            if res[0] == "pil":
                return _into(torch.from_numpy(res[1]).to(self.device, non_blocking=True), out)
            _, geom, coef = res
            if not self._cuda:
                return _into(torch.from_numpy(ops.jpeg_pixels_host(coef, geom)), out)
            coef_d = coef.to(self.device, non_blocking=True)
            slot = self._slots[k]
            if slot.ev is None:
                slot.ev = torch.cuda.Event()
            slot.ev.record(torch.cuda.current_stream())
            return _pixels(coef_d, geom, out)
        finally:
            self._free.append(k)

    def close(self):
        for fut, _ in self._pending.values():
            fut.cancel()
        self._pool.shutdown(wait=True)
        self._pending = {}


def encode_bgr(im, quality=90, subsampling=2):
    """BGR uint8 [h,w,3] -> the bytes of a baseline JPEG file whose coefficients are those of PIL's encoder at the same quality and
    subsampling (0 / 1 / 2 = 4:4:4 / 4:2:2 / 4:2:0).  A device tensor: colour conversion, downsampling, DCT and quantisation in two launches,
    the coefficient buffer copied to the host, the Huffman stage there.  A CPU tensor or numpy array: the host statement of the kernels."""
    if torch.is_tensor(im) and im.is_cuda:
        coef = ops.jpeg_coefs(im, quality, subsampling).cpu()
    else:
        coef = ops.jpeg_coefs_host(im, quality, subsampling)
    return ops.jpeg_entropy_encode(coef, ops.jpeg_encode_geom(im.shape[0], im.shape[1], subsampling))


class _WSlot(object):
    __slots__ = ("buf", "ev", "fut")

    def __init__(self):
        self.buf, self.ev, self.fut = None, None, None


class JpegWriter(object):
    """The counterpart of JpegCache: submit(path, im_d) launches the two encode kernels on the caller's current stream, copies the
    coefficient buffer into one of `depth` pinned buffers and records an event; a worker thread waits for the event, runs the Huffman stage
    (C, the GIL released) and writes the file.  A pinned buffer is used again only after its file has been written.  An exception of a worker
    (an unwritable path, say) is raised by the next submit() or by close()."""

    MIN_SLOT_BYTES = 1 << 20

    def __init__(self, device, workers=4, depth=8):
        self.device = torch.device(device)
        self._cuda = _is_cuda(device)
        self._pool = ThreadPoolExecutor(max_workers=max(1, min(int(workers), MAX_WORKERS)))
        self._slots = [_WSlot() for _ in range(max(1, int(depth)))]
        self._k = 0
        self._errors = []

    def _work(self, path, slot, nbytes, geom):
        if slot.ev is not None:
            slot.ev.synchronize()                                # the copy into this buffer has finished
        data = ops.jpeg_entropy_encode(slot.buf[:nbytes], geom)
        with open(path, "wb") as f:
            f.write(data)

    def _reap(self, slot):
        """wait until the slot's file is written; keep a worker's exception for _raise"""
        fut, slot.fut = slot.fut, None
        if fut is not None:
            try:
                fut.result()
            except Exception as e:                               # noqa: BLE001  (re-raised by _raise)
                self._errors.append(e)

    def _raise(self):
        if self._errors:
            e, self._errors = self._errors[0], []
            raise e

    def submit(self, path, im, quality=90, subsampling=2):
        for s in self._slots:                                    # whatever has finished by now, without waiting
            if s.fut is not None and s.fut.done():
                self._reap(s)
        self._raise()
        slot = self._slots[self._k]
        self._k = (self._k + 1) % len(self._slots)
        self._reap(slot)
        self._raise()
        geom = ops.jpeg_encode_geom(im.shape[0], im.shape[1], subsampling)
        n = ops.jpeg_coef_bytes(geom)
        if slot.buf is None or slot.buf.numel() < n:
            slot.buf = torch.empty(max(n, self.MIN_SLOT_BYTES), dtype=torch.uint8, pin_memory=self._cuda)
        if self._cuda:
            slot.buf[:n].copy_(ops.jpeg_coefs(im, quality, subsampling), non_blocking=True)
            if slot.ev is None:
                slot.ev = torch.cuda.Event()
            slot.ev.record(torch.cuda.current_stream())
        else:
            ops.jpeg_coefs_host(im, quality, subsampling, out=slot.buf)
        slot.fut = self._pool.submit(self._work, path, slot, n, geom)

    def close(self):
        for s in self._slots:
            self._reap(s)
        self._pool.shutdown(wait=True)
        self._raise()


class JpegPrefetcher(object):
    """Ordered iterator over `paths` (file paths or bytes objects) -> BGR uint8 [h,w,3] tensors on `device`; up to `depth` files are read and
    entropy-decoded ahead by `workers` threads (a plain argument, capped at 8)."""

    def __init__(self, paths, device, workers=4, depth=8):
        self._paths = list(paths)
        self._cache = JpegCache(device, workers=workers, depth=depth)
        self._depth = max(1, int(depth))
        self._i = 0
        self._ahead = 0
        self._fill()

    def _fill(self):
        self._ahead = max(self._ahead, self._i)
        while self._ahead < min(len(self._paths), self._i + self._depth) and self._cache.prefetch(self._ahead, self._paths[self._ahead]):
            self._ahead += 1

    def __len__(self):
        return len(self._paths)

    def __iter__(self):
        return self

    def __next__(self):
        return self.read_into(None)

    next = __next__

    def read_into(self, out):
        """the next image decoded INTO `out` ([h,w,3] uint8 on the device, e.g. one slot of a batch buffer); None: a new tensor"""
        if self._i >= len(self._paths):
            self._cache.close()
            raise StopIteration
        i = self._i
        self._i += 1
        try:
            return self._cache.get(i, self._paths[i], out)
        finally:
            self._fill()

    def close(self):
        self._cache.close()
