"""Batch preparation on the GPU: decoded uint8 RGB images in, the model's padded fp32 batch out.

One kernel launch per batch (csrc/image.hip, dadet_image_prepare_batch) replaces the reference's per-sample host chain Resize ->
RandomHorizontalFlip -> RandomVerticalFlip -> ToTensor -> Normalize (data/transforms/transforms.py:32-97) and the collator's
zero padding (data/collate_batch.py:46-55, structures/image_list.py:49-91); where the chain starts with a ColorJitter, at
most two more launches per batch apply it to the decoded pixels first (csrc/color_jitter.hip, data/color_jitter.py).  The resize is Pillow's bilinear resample reproduced bit
for bit (integer arithmetic), so the batch equals what the host transforms produce; ground-truth boxes are resized /
mirrored by the same BoxList methods the reference calls.  Random decisions (jitter, training scale, flips) are drawn from
Python's `random` in the host chain's per-sample order (data/transforms.py draw_decisions) — by the preparer itself, or (the
loaders of data/build.py with device_prep=True) inside the dataset's __getitem__, where the host chain draws them.
`DevicePrepLoader` puts a raw DataLoader and a preparer behind the interface of the host loaders."""
import collections
import ctypes
import math

import numpy as np
import torch

from .. import _lib
from ..structures.image_list import ImageList
from .datasets import RainImage, RainyDataset, RawImage
from .color_jitter import jitter_device
from .transforms import build_transforms, draw_decisions, split_decision

_PRECISION_BITS = 32 - 8 - 2
_TABLES = {}


def resample_tables(in_size, out_size):
    """Pillow's per-axis tables (Resample.c precompute_coeffs + normalize_coeffs_8bpc, bilinear filter): bounds
    int32 [out,2] = (first input index, tap count), coefficients int32 [out,ksize] in 2^-22 units."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    xx = np.arange(out_size, dtype=np.float64)
    center = (xx + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)          # C truncation of a value > -1
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size)
    n = xmax - xmin
    taps = np.arange(ksize, dtype=np.float64)[None, :]
    w = np.abs((taps + xmin[:, None] - center[:, None] + 0.5) * (1.0 / filterscale))
    w = np.where(w < 1.0, 1.0 - w, 0.0)
    w = np.where(taps < n[:, None], w, 0.0)
    # Pillow sums the weights left to right in double precision; cumsum reproduces that order
    ww = np.cumsum(w, axis=1)[:, -1:]
    k = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    coeffs = (k * float(1 << _PRECISION_BITS) + 0.5).astype(np.int64).astype(np.int32)   # weights are >= 0
    bounds = np.stack([xmin, n], axis=1).astype(np.int32)
    return bounds, coeffs


def _device_tables(in_size, out_size, device):
    key = (in_size, out_size, str(device))
    if key not in _TABLES:
        b, c = resample_tables(in_size, out_size)
        if len(_TABLES) > 64:
            _TABLES.clear()
        _TABLES[key] = (torch.from_numpy(b).to(device), torch.from_numpy(c).to(device), c.shape[1])
    return _TABLES[key]


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def resize_normalize_into(image_u8, out_hw, flip, mean, std, to_bgr255, out_slot):
    """image_u8 [H,W,3] uint8 on the device, flip a bool or a mask of _lib.FLIP_H / FLIP_V -> writes fp32 into out_slot, a [3, Hp, Wp] channels_last view (physically
    [Hp][Wp][3]) with Hp >= oh, Wp >= ow; everything outside [oh, ow] is left untouched (zero padding)"""
    if not image_u8.is_cuda:
        raise _lib.DadetError("resize_normalize_into: the image must live on the HIP device")
    assert image_u8.dtype == torch.uint8 and image_u8.dim() == 3 and image_u8.shape[2] == 3
    image_u8 = image_u8.contiguous()
    H, W = int(image_u8.shape[0]), int(image_u8.shape[1])
    oh, ow = out_hw
    dev = image_u8.device
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    cur = image_u8
    if ow != W:
        bw, cw, kw = _device_tables(W, ow, dev)
        tmp = torch.empty((H, ow, 3), dtype=torch.uint8, device=dev)
        _lib.call("dadet_image_resample_h", _p(cur), H, W, _p(bw), _p(cw), kw, ow, _p(tmp), stream)
        cur = tmp
    bh = ch = None
    kh = 0
    if oh != H:
        bh, ch, kh = _device_tables(H, oh, dev)
    assert out_slot.stride(0) == 1 and out_slot.stride(2) == 3, "out_slot must be a channels_last [3,Hp,Wp] view"
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in std])
    _lib.call("dadet_image_resample_v_normalize", _p(cur), H, ow, _p(bh), _p(ch), kh, oh, int(flip),
              int(bool(to_bgr255)), m, s, _p(out_slot), int(out_slot.stride(1) // 3), stream)


class DeviceBatchPreparer(object):
    """callable(images_u8, targets=None) -> (ImageList, targets): the GPU counterpart of `build_transforms(cfg)`
    followed by `BatchCollator(cfg.DATALOADER.SIZE_DIVISIBILITY)`."""

    def __init__(self, cfg, is_train=True):
        self.transforms = build_transforms(cfg, is_train)          # for its draws alone: nothing of it is applied
        self.mean, self.std = cfg.INPUT.PIXEL_MEAN, cfg.INPUT.PIXEL_STD
        self.to_bgr255 = cfg.INPUT.TO_BGR255
        self.size_divisible = cfg.DATALOADER.SIZE_DIVISIBILITY

    def __call__(self, images_u8, targets=None, decisions=None):
        """images_u8: list of uint8 [H,W,3] RGB device tensors, or of the loaders' `RawImage` (device pixels with the
        decisions drawn in the dataset).  decisions (optional): list of ((oh, ow), flip) or ((oh, ow), flip, vertical
        flip, jitter operators) — data/transforms.py draw_decisions — to use instead of those, or instead of drawing them
        here.  Images whose decision carries jitter operators are jittered on the current stream first."""
        if decisions is None and all(isinstance(im, RawImage) for im in images_u8):
            decisions = [im.decision for im in images_u8]
        images_u8 = [im.pixels if isinstance(im, RawImage) else im for im in images_u8]
        n = len(images_u8)
        if decisions is None:
            decisions = []
            # per sample, in the order of the chain's steps (transforms/build.py:36-45)
            decisions = [draw_decisions(self.transforms, (int(img.shape[1]), int(img.shape[0]))) for img in images_u8]
        images_u8 = jitter_device(images_u8, [split_decision(d)[3] for d in decisions])
        sizes = [d[0] for d in decisions]
        hp, wp = max(s[0] for s in sizes), max(s[1] for s in sizes)
        if self.size_divisible > 0:
            d = self.size_divisible
            hp, wp = int(math.ceil(hp / d) * d), int(math.ceil(wp / d) * d)
        dev = images_u8[0].device
        # (no clearing pass: the kernel writes the padding of every slot itself)
        batch = torch.empty((n, 3, hp, wp), dtype=torch.float32, device=dev, memory_format=torch.channels_last)
        prepare_batch_into(images_u8, decisions, self.mean, self.std, self.to_bgr255, batch)
        return ImageList(batch, [(oh, ow) for (oh, ow) in sizes]), self.transform_targets(targets, decisions)

    @staticmethod
    def transform_targets(targets, decisions):
        """the boxes follow their image through the BoxList methods the host transforms call"""
        if targets is None:
            return None
        out = []
        for t, decision in zip(targets, decisions):
            (oh, ow), flip, vflip, _ = split_decision(decision)
            t = t.resize((ow, oh))
            t = t.transpose(0) if flip else t
            out.append(t.transpose(1) if vflip else t)
        return out


def prepare_batch_into(images_u8, decisions, mean, std, to_bgr255, batch):
    """images_u8: uint8 [H,W,3] device tensors; decisions: ((oh, ow), flip[, vertical flip, ...]) per image; batch: fp32 [n,3,Hp,Wp]
    channels_last on the same device, uninitialised.  One launch per _lib.IMAGE_BATCH_MAX images (dadet_image_prepare_batch)
    on the current stream writes image i, resized / mirrored / normalised, into batch[i] and zeros around it.  (The jitter
    operators of a long decision are the caller's to apply: DeviceBatchPreparer does, ahead of this.)"""
    n, _, hp, wp = (int(v) for v in batch.shape)
    if not batch.is_cuda or any(not im.is_cuda for im in images_u8):
        raise _lib.DadetError("prepare_batch_into: images and batch must live on the HIP device")
    assert len(images_u8) == len(decisions) == n and batch.dtype == torch.float32
    assert batch.stride(1) == 1 and batch.stride(3) == 3 and batch.stride(2) == 3 * wp and (
        n == 1 or batch.stride(0) == 3 * hp * wp), "batch must be a dense channels_last [n,3,Hp,Wp] tensor"
    dev = batch.device
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in std])
    keep = []          # contiguous copies stay alive until their launch is issued (stream-ordered allocator after that)
    for first in range(0, n, _lib.IMAGE_BATCH_MAX):
        count = min(_lib.IMAGE_BATCH_MAX, n - first)
        items = (_lib.ImageItem * count)()
        for j in range(count):
            img, ((oh, ow), flip, vflip, _) = images_u8[first + j], split_decision(decisions[first + j])
            assert img.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == 3 and img.device == dev
            img = img.contiguous()
            keep.append(img)
            H, W = int(img.shape[0]), int(img.shape[1])
            it = items[j]
            it.src, it.H, it.W, it.out_h, it.out_w = img.data_ptr(), H, W, int(oh), int(ow)
            it.flip, it.slot = (_lib.FLIP_H if flip else 0) | (_lib.FLIP_V if vflip else 0), first + j
            if ow != W:
                bw, cw, it.h_ksize = _device_tables(W, int(ow), dev)
                it.h_bounds, it.h_coeffs = bw.data_ptr(), cw.data_ptr()
                keep += [bw, cw]
            if oh != H:
                bh, ch, it.v_ksize = _device_tables(H, int(oh), dev)
                it.v_bounds, it.v_coeffs = bh.data_ptr(), ch.data_ptr()
                keep += [bh, ch]
        _lib.call("dadet_image_prepare_batch", items, count, int(bool(to_bgr255)), m, s, _p(batch), n, hp, wp, stream)
    # pixels and (cached) tables may have been allocated on another stream than the one that reads them here
    cur = torch.cuda.current_stream(dev)
    for t in keep:
        t.record_stream(cur)


class _Staging(object):
    """one pinned host buffer and the event of the last upload that read it"""

    def __init__(self):
        self.buffer, self.event = None, None

    def take(self, nbytes):
        if self.event is not None:
            self.event.synchronize()           # the upload that last read this buffer has finished
        if self.buffer is None or self.buffer.numel() < nbytes:
            self.buffer = torch.empty(max(nbytes, 1), dtype=torch.uint8).pin_memory()
        return self.buffer


class DevicePrepLoader(object):
    """A raw `DataLoader` (decode_to_tensor datasets, one of the Raw* collators of data/collate_batch.py) and a
    `DeviceBatchPreparer` behind the interface of the host loaders: `len`, `dataset`, `batch_sampler`, `collate_fn`, and
    batches of (ImageList, targets, ids) — nine fields from the triplet collator — with images and targets already on
    the device.  From the test-time-augmentation collator the batches stay (images, targets, ids) with the images as
    uint8 device tensors, uploaded once: every pass of engine/bbox_aug.py prepares its own input from them.

    One batch of look-ahead: batch k + 1 is fetched from the workers, copied into a pinned staging buffer (in this
    process: the workers never touch the device), uploaded with non_blocking=True and prepared on a side stream before batch
    k is handed out, so upload and preparation run beside the step that is still executing; the consumer's stream waits
    for the batch's event when it receives it.  Two staging buffers take turns, each reused only after the upload that
    read it has finished (its event); the device tensors are allocated on the side stream and registered with the
    consumer's stream at the hand-over (record_stream), so the allocator does not recycle them while either stream may
    still use them.  Loaders read side by side are joined with `consumed_jointly`.

    Samples of a RainyDataset (`RainImage`: source pixels + rain mask index + plan) become their rainy image on the side
    stream before the preparation launch (data/rain.py synthesize_device); pixels two samples share — an aligned triplet's
    source and rainy sample — are copied and uploaded once.  The colour jitter of a sample's decision follows, on the same
    stream and into a buffer of its own (the preparer applies it): the rainy sample is jittered as a rainy image, like on
    the host chain, and two samples that share an upload may draw different jitters."""

    SIDE_STREAM = 3            # utils/streams.py: 0 / 1 bookkeeping sections, 2 the weight-gradient lane

    def __init__(self, loader, preparer, device=None):
        self.loader, self.preparer = loader, preparer
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None and torch.cuda.is_available() \
            else (torch.device(device) if device is not None else None)
        self._staging = [_Staging(), _Staging()]
        self._turn = 0
        self._group = [self]
        self._started, self._source, self._queue = False, None, collections.deque()

    @staticmethod
    def consumed_jointly(loaders):
        """The loaders of one training loop (source, target, auxiliary: do_da_train takes one batch of each per step).
        With DATALOADER.NUM_WORKERS 0 their samples draw from ONE random stream, in the order the batches are fetched; a
        look-ahead of each loader on its own would fetch source batch 1 before target batch 0 and so change every draw
        after the first batch.  Joined, they fetch in rounds — one batch of every loader, in this order — which is the
        order the host loaders are read in, look-ahead or not."""
        for loader in loaders:
            loader._group = list(loaders)
        return loaders

    dataset = property(lambda self: self.loader.dataset)
    batch_sampler = property(lambda self: self.loader.batch_sampler)
    collate_fn = property(lambda self: self.loader.collate_fn)

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        if self.device is None or self.device.type != "cuda":
            raise _lib.DadetError("DevicePrepLoader needs a HIP device: the preparation has no CPU fallback")
        if not self._started:                      # (a member of a group may have been started by another member)
            for member in self._group:
                if not member._started:
                    member._started, member._source = True, iter(member.loader)
                    member._queue.clear()
        try:
            while True:
                # the batch handed out next and one of look-ahead; a round fetches one batch of every member of the group
                while len(self._queue) < 2 and self._source is not None:
                    for member in self._group:
                        member._fetch_one()
                if not self._queue:
                    return
                yield self._hand_over(self._queue.popleft())
        finally:
            self._started, self._source = False, None
            self._queue.clear()

    def _fetch_one(self):
        if self._source is None:
            return
        try:
            raw = next(self._source)
        except StopIteration:
            self._source = None
            return
        self._queue.append(self._stage(raw))

    # ------------------------------------------------------------------------------------------------------------
    def _upload(self, images, side):
        """every image of the batch through ONE pinned buffer and ONE copy -> per-image device views (same kind as given:
        RawImage or bare pixels)"""
        pixels = [im.pixels if isinstance(im, RawImage) else im for im in images]
        offsets, total, seen = [], 0, {}
        for p in pixels:
            assert p.dtype == torch.uint8 and p.dim() == 3 and p.shape[2] == 3 and not p.is_cuda
            # an aligned triplet's rainy sample carries the source sample's own tensor: one copy, one upload, two views
            key = (p.data_ptr(), tuple(p.shape), p.stride())
            if key not in seen:
                seen[key] = total
                total += (p.numel() + 255) // 256 * 256
            offsets.append(seen[key])
        stage = self._staging[self._turn]
        self._turn ^= 1
        host = stage.take(total)
        for off, p in {off: p for p, off in zip(pixels, offsets)}.items():
            host[off:off + p.numel()].view(p.shape).copy_(p)
        with torch.cuda.stream(side):
            dev = host[:total].to(self.device, non_blocking=True)
            stage.event = side.record_event()
        views = [dev[off:off + p.numel()].view(p.shape) for p, off in zip(pixels, offsets)]
        return [RawImage(v, im.decision) if isinstance(im, RawImage) else v for v, im in zip(views, images)]

    def _rain_masks(self):
        dataset = self.loader.dataset
        for part in (dataset, getattr(dataset, "dataset_n", None)):
            if isinstance(part, RainyDataset):
                return part.masks
        raise _lib.DadetError("a rainy sample arrived from a loader without a RainyDataset")

    def _rain(self, sample, uploaded):
        """a RainyDataset sample whose SOURCE pixels are on the device -> RawImage of the rainy image, synthesised on the
        current (side) stream (data/rain.py synthesize_device); the mask comes from the masks' device cache"""
        from .rain import synthesize_device

        H, W = int(uploaded.pixels.shape[0]), int(uploaded.pixels.shape[1])
        mask = self._rain_masks().device_mask(sample.mask_index, (W, H), self.device)
        return RawImage(synthesize_device(uploaded.pixels, mask, sample.plan), uploaded.decision)

    def _stage(self, raw):
        from ..utils.streams import side_stream

        side = side_stream(self.device, self.SIDE_STREAM)
        groups = (0,) if len(raw) == 3 else (0, 2, 4)             # (images, targets) field pairs of the batch
        counts = [len(raw[g]) for g in groups]
        flat = [im for g in groups for im in raw[g]]
        uploaded = self._upload(flat, side)
        out = list(raw)
        source_decisions = None
        with torch.cuda.stream(side):
            uploaded = [self._rain(im, up) if isinstance(im, RainImage) else up for im, up in zip(flat, uploaded)]
            for g, first in zip(groups, np.cumsum([0] + counts[:-1])):
                images = uploaded[first:first + len(raw[g])]
                if not all(isinstance(im, RawImage) for im in images):
                    out[g] = images                               # test-time augmentation: the pixels themselves
                    continue
                decisions = [im.decision for im in images]
                # the boxes are transformed on the host, like the host chain's.  An aligned triplet's target / auxiliary
                # annotations are copies of the SOURCE sample's (TripletDataset._with_domain), which the host chain takes
                # after the source sample's transforms: they follow the source image's decisions, not their own image's
                source_decisions = source_decisions or decisions
                targets = self.preparer.transform_targets(list(raw[g + 1]), source_decisions)
                out[g], _ = self.preparer(images, None, decisions)
                out[g + 1] = tuple(t.to(self.device) for t in targets)
            done = side.record_event()
        return tuple(out), done

    def _hand_over(self, staged):
        from ..utils.streams import record

        batch, done = staged
        main = torch.cuda.current_stream(self.device)
        main.wait_event(done)
        for field in batch:
            record(field.tensors if isinstance(field, ImageList) else field, main)
        return batch
