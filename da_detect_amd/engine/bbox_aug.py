"""Test-time box augmentation (reference: maskrcnn_benchmark/engine/bbox_aug.py:11-118 of the vendored tree): the model
runs on the image as it is, on its mirror image and on rescaled copies, every pass's unfiltered detections are brought
back to the first pass's frame, concatenated per image and filtered ONCE (threshold, per-class NMS, cut) — the merged
list of several thousand rows goes through the device filter like any other (csrc/detect_post.hip).

The passes build their inputs with this package's own sample transforms (data/transforms.py: Pillow + torch).  The
configuration is the one the model was built from (`model.cfg`); a model without one — the reference's own tools merge
into the package-level `cfg` — falls back to that, read at call time.

Images given as uint8 [H,W,3] tensors (the RawBBoxAugCollator of a `device_prep` loader) instead of PIL images take the
device path: each image is uploaded once — by the loader, else here — and every pass is one batched preparation launch
(data/device_prep.py) with that pass's size and flip; no PIL resize and no further upload per pass.  Same bits."""
import torch

from ..data import transforms as T
from ..modeling.roi_heads.box_head.inference import make_roi_box_post_processor
from ..structures.bounding_box import BoxList
from ..structures.image_list import to_image_list


def _cfg_of(model):
    cfg = getattr(getattr(model, "module", model), "cfg", None)
    if cfg is None:
        from ..config import cfg
    return cfg


def im_detect_bbox_aug(model, images, device):
    """bbox_aug.py:11-68: identity, flip (H_FLIP), then per scale the plain and (SCALE_H_FLIP) the flipped pass"""
    cfg = _cfg_of(model)
    if _is_raw(images):
        images = [image.to(device, non_blocking=True) for image in images]      # once for all passes
    boxlists_ts = [[] for _ in range(len(images))]

    def add_preds_t(boxlists_t):
        for i, boxlist_t in enumerate(boxlists_t):
            # the first pass is the identity: every later one is resized to its frame
            boxlists_ts[i].append(boxlist_t if not boxlists_ts[i] else boxlist_t.resize(boxlists_ts[i][0].size))

    add_preds_t(im_detect_bbox(model, images, cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST, device))
    if cfg.TEST.BBOX_AUG.H_FLIP:
        add_preds_t(im_detect_bbox_hflip(model, images, cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST, device))
    for scale in cfg.TEST.BBOX_AUG.SCALES:
        max_size = cfg.TEST.BBOX_AUG.MAX_SIZE
        add_preds_t(im_detect_bbox_scale(model, images, scale, max_size, device))
        if cfg.TEST.BBOX_AUG.SCALE_H_FLIP:
            add_preds_t(im_detect_bbox_scale(model, images, scale, max_size, device, hflip=True))

    merged = []
    for boxlist_ts in boxlists_ts:
        boxlist = BoxList(torch.cat([b.bbox for b in boxlist_ts]), boxlist_ts[0].size, boxlist_ts[0].mode)
        boxlist.add_field("scores", torch.cat([b.get_field("scores") for b in boxlist_ts]))
        merged.append(boxlist)
    post_processor = make_roi_box_post_processor(cfg)
    num_classes = cfg.MODEL.ROI_BOX_HEAD.NUM_CLASSES
    return [post_processor.filter_results(boxlist, num_classes) for boxlist in merged]


def _is_raw(images):
    return len(images) > 0 and all(isinstance(im, torch.Tensor) and im.dtype == torch.uint8 for im in images)


def _detect_raw(model, images, target_scale, target_max_size, device, hflip, cfg):
    """one pass on decoded uint8 pixels: the pass's (Resize.get_size, flip) for every image, one launch"""
    from ..data.device_prep import DeviceBatchPreparer

    resize = T.Resize(target_scale, target_max_size)
    decisions = [(resize.get_size((int(im.shape[1]), int(im.shape[0]))), bool(hflip)) for im in images]
    batch, _ = DeviceBatchPreparer(cfg, is_train=False)([im.to(device) for im in images], None, decisions)
    return model(batch)


def _detect(model, images, target_scale, target_max_size, device, hflip):
    cfg = _cfg_of(model)
    if _is_raw(images):
        return _detect_raw(model, images, target_scale, target_max_size, device, hflip, cfg)
    steps = [T.Resize(target_scale, target_max_size)]
    if hflip:
        steps.append(T.RandomHorizontalFlip(1.0))
    steps += [T.ToTensor(), T.Normalize(mean=cfg.INPUT.PIXEL_MEAN, std=cfg.INPUT.PIXEL_STD, to_bgr255=cfg.INPUT.TO_BGR255)]
    transform = T.Compose(steps)
    tensors = [transform(image, None)[0] for image in images]
    return model(to_image_list(tensors, cfg.DATALOADER.SIZE_DIVISIBILITY).to(device))


def im_detect_bbox(model, images, target_scale, target_max_size, device):
    """detection on the image as it is (bbox_aug.py:71-84)"""
    return _detect(model, images, target_scale, target_max_size, device, False)


def im_detect_bbox_hflip(model, images, target_scale, target_max_size, device):
    """detection on the mirror image, the boxes mirrored back (bbox_aug.py:87-106)"""
    return [boxlist.transpose(0) for boxlist in _detect(model, images, target_scale, target_max_size, device, True)]


def im_detect_bbox_scale(model, images, target_scale, target_max_size, device, hflip=False):
    """detection at another scale, in the scaled image's frame (bbox_aug.py:109-118)"""
    if hflip:
        return im_detect_bbox_hflip(model, images, target_scale, target_max_size, device)
    return im_detect_bbox(model, images, target_scale, target_max_size, device)
