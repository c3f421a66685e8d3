"""PASCAL VOC scoring: AP at one or several IoU thresholds, matched on the device (voc_eval.py, csrc/voc_match.hip)."""
import logging

from .voc_eval import do_voc_evaluation


def voc_evaluation(dataset, predictions, output_folder, box_only=False, iou_thresh=0.5, use_07_metric=True, **_):
    """the keyword form `evaluate` hands on; `box_only` and the COCO arguments (`iou_types`, ...) mean nothing here"""
    logger = logging.getLogger("maskrcnn_benchmark.inference")
    if box_only:
        logger.warning("voc evaluation doesn't support box_only, ignored.")
    logger.info("performing voc evaluation, ignored iou_types.")
    return do_voc_evaluation(dataset=dataset, predictions=predictions, output_folder=output_folder, logger=logger,
                             iou_thresh=iou_thresh, use_07_metric=use_07_metric)
