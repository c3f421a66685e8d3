"""COCO-style scoring: box AP on the device and proposal recall on the host (coco_eval.py, box_ap.py)."""
from .coco_eval import do_coco_evaluation


def coco_evaluation(dataset, predictions, output_folder, box_only, iou_types, expected_results,
                    expected_results_sigma_tol):
    """the keyword form `evaluate` hands on, in do_coco_evaluation's positional order"""
    return do_coco_evaluation(dataset, predictions, box_only, output_folder, iou_types, expected_results,
                              expected_results_sigma_tol)
