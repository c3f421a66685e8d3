"""Detection post-processing for evaluation (reference:
maskrcnn_benchmark/modeling/roi_heads/box_head/inference.py:12-150): softmax, per-class decode, clip,
score threshold, per-class NMS (HIP), top detections_per_img.

The filter (threshold, per-class NMS, order, cut) runs on the device for a whole batch in one fixed sequence of launches
(csrc/detect_post.hip); the reference's per-class Python loop stays for CPU tensors and behind DADET_DEVICE_POSTPROCESS=0."""
import os

import torch
import torch.nn.functional as F
from torch import nn

from .... import _C
from ....structures.bounding_box import BoxList
from ....structures.boxlist_ops import boxlist_nms, cat_boxlist
from ...box_coder import BoxCoder


class PostProcessor(nn.Module):
    def __init__(self, score_thresh=0.05, nms=0.5, detections_per_img=100, box_coder=None,
                 cls_agnostic_bbox_reg=False, bbox_aug_enabled=False):
        super(PostProcessor, self).__init__()
        self.score_thresh = score_thresh
        self.nms = nms
        self.detections_per_img = detections_per_img
        self.box_coder = box_coder if box_coder is not None else BoxCoder(weights=(10.0, 10.0, 5.0, 5.0))
        self.cls_agnostic_bbox_reg = cls_agnostic_bbox_reg
        self.bbox_aug_enabled = bbox_aug_enabled

    def forward(self, x, boxes):
        class_logits, box_regression = x
        class_prob = F.softmax(class_logits, -1)
        counts = [len(b) for b in boxes]
        concat_boxes = torch.cat([b.bbox for b in boxes], dim=0)
        if self.cls_agnostic_bbox_reg:
            box_regression = box_regression[:, -4:]
        proposals = self.box_coder.decode(box_regression.reshape(sum(counts), -1), concat_boxes)
        if self.cls_agnostic_bbox_reg:
            proposals = proposals.repeat(1, class_prob.shape[1])
        num_classes = class_prob.shape[1]
        clipped = []
        for prob, boxes_per_img, box in zip(class_prob.split(counts, dim=0), proposals.split(counts, dim=0), boxes):
            boxlist = BoxList(boxes_per_img.reshape(-1, 4), box.size, mode="xyxy")
            boxlist.add_field("scores", prob.reshape(-1))
            clipped.append(boxlist.clip_to_image(remove_empty=False))
        if self.bbox_aug_enabled:       # test-time augmentation filters the merged passes itself (inference.py:84)
            return clipped
        return self.filter_batch(clipped, num_classes)

    def _on_device(self, boxlists, num_classes):
        """the device filter takes this batch: device tensors, the switch not at 0, every image within the ranked-set limit"""
        if os.environ.get("DADET_DEVICE_POSTPROCESS", "1") == "0":          # read per call
            return False
        return all(b.bbox.is_cuda and b.bbox.dtype == torch.float32 and
                   b.bbox.shape[0] // num_classes <= _C.NMS_BATCH_MAX_BOXES for b in boxlists)

    def filter_batch(self, boxlists, num_classes):
        """filter_results for the images of a batch: one call of the device filter instead of one loop per image"""
        if not boxlists or not self._on_device(boxlists, num_classes):
            return [self._filter_results_loop(b, num_classes) for b in boxlists]
        results = []
        for i in range(0, len(boxlists), _C.DETECT_POST_MAX_IMAGES):
            part = boxlists[i:i + _C.DETECT_POST_MAX_IMAGES]
            rows = [b.bbox.shape[0] // num_classes for b in part]
            boxes = torch.cat([b.bbox for b in part], dim=0) if len(part) > 1 else part[0].bbox
            scores = torch.cat([b.get_field("scores") for b in part], dim=0) if len(part) > 1 else part[0].get_field("scores")
            dets = _C.detect_post(boxes.reshape(-1, num_classes, 4), scores.reshape(-1, num_classes), rows, self.score_thresh,
                                  self.nms, self.detections_per_img)
            for b, (det_boxes, det_scores, det_labels) in zip(part, dets):
                result = BoxList(det_boxes, b.size, mode="xyxy")
                result.add_field("scores", det_scores)
                result.add_field("labels", det_labels)
                results.append(result)
        return results

    def filter_results(self, boxlist, num_classes):
        return self.filter_batch([boxlist], num_classes)[0]

    def _filter_results_loop(self, boxlist, num_classes):
        """the reference's loop (inference.py:108-149): the path of CPU tensors, of lists beyond the device filter's limit,
        and the yardstick the device filter is tested and timed against"""
        boxes = boxlist.bbox.reshape(-1, num_classes * 4)
        scores = boxlist.get_field("scores").reshape(-1, num_classes)
        device = scores.device
        above = scores > self.score_thresh
        per_class = []
        for j in range(1, num_classes):  # class 0 is background
            inds = above[:, j].nonzero().squeeze(1)
            bl = BoxList(boxes[inds, j * 4:(j + 1) * 4], boxlist.size, mode="xyxy")
            bl.add_field("scores", scores[inds, j])
            bl = boxlist_nms(bl, self.nms)
            bl.add_field("labels", torch.full((len(bl),), j, dtype=torch.int64, device=device))
            per_class.append(bl)
        result = cat_boxlist(per_class)
        n = len(result)
        if n > self.detections_per_img > 0:
            cls_scores = result.get_field("scores")
            thresh, _ = torch.kthvalue(cls_scores.cpu(), n - self.detections_per_img + 1)
            result = result[torch.nonzero(cls_scores >= thresh.item()).squeeze(1)]
        return result


def make_roi_box_post_processor(cfg):
    box_coder = BoxCoder(weights=cfg.MODEL.ROI_HEADS.BBOX_REG_WEIGHTS)
    return PostProcessor(cfg.MODEL.ROI_HEADS.SCORE_THRESH, cfg.MODEL.ROI_HEADS.NMS,
                         cfg.MODEL.ROI_HEADS.DETECTIONS_PER_IMG, box_coder, cfg.MODEL.CLS_AGNOSTIC_BBOX_REG,
                         cfg.TEST.BBOX_AUG.ENABLED)
