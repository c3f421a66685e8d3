"""Scoring of an inference pass on a COCO-style dataset (reference: data/datasets/evaluation/coco/coco_eval.py).

What the reference hands to pycocotools — once per category and once for all of them — is one matching launch on the
device here (box_ap.py, csrc/coco_match.hip), from which the six numbers for all categories and the six per category both
come.  Proposal recall is plain torch on the host, as in the reference.  Masks and keypoints are outside this package."""
import collections
import json
import logging
import os

import torch

from ....structures.bounding_box import BoxList
from ....structures.boxlist_ops import boxlist_iou
from . import box_ap

PROPOSAL_AREAS = collections.OrderedDict([
    ("all", (0 ** 2, 1e5 ** 2)), ("small", (0 ** 2, 32 ** 2)), ("medium", (32 ** 2, 96 ** 2)), ("large", (96 ** 2, 1e5 ** 2)),
    ("96-128", (96 ** 2, 128 ** 2)), ("128-256", (128 ** 2, 256 ** 2)), ("256-512", (256 ** 2, 512 ** 2)),
    ("512-inf", (512 ** 2, 1e5 ** 2))])


class _ConcatView(object):
    """a ConcatDataset of COCODatasets seen as one: the members prepare_for_coco_detection, box_ap.pack and
    evaluate_box_proposals touch.  Image ids must not repeat across the parts (a record names its image by id alone)."""

    def __init__(self, concat):
        parts = list(concat.datasets)
        self.ids = [i for d in parts for i in d.ids]
        if len(set(self.ids)) != len(self.ids):
            raise ValueError("the concatenated datasets share image ids; their detections cannot be told apart")
        self.id_to_img_map = dict(enumerate(self.ids))
        self.anns_of = {i: d.anns_of[i] for d in parts for i in d.ids if i in d.anns_of}
        self.contiguous_category_id_to_json_id = parts[0].contiguous_category_id_to_json_id
        if any(d.contiguous_category_id_to_json_id != self.contiguous_category_id_to_json_id for d in parts):
            raise ValueError("the concatenated datasets have different categories")
        self.get_img_info = concat.get_img_info


def _as_one(dataset):
    return _ConcatView(dataset) if isinstance(dataset, torch.utils.data.ConcatDataset) else dataset


def do_coco_evaluation(dataset, predictions, box_only, output_folder, iou_types, expected_results,
                       expected_results_sigma_tol):
    """box_only: proposal recalls (AR at 100 and 1000 proposals, four area ranges), saved as box_proposals.pth, returns
    None.  Otherwise: the bbox records (bbox.json), box AP for all categories and per category (coco_results.pth), returns
    (COCOResults, {"bbox": records})."""
    from ....engine.inference import prepare_for_coco_detection

    log = logging.getLogger("maskrcnn_benchmark.inference")
    dataset = _as_one(dataset)
    if box_only:
        log.info("Evaluating bbox proposals")
        res = COCOResults("box_proposal")
        for limit in (100, 1000):
            for area, suffix in (("all", ""), ("small", "s"), ("medium", "m"), ("large", "l")):
                stats = evaluate_box_proposals(predictions, dataset, area=area, limit=limit)
                res.results["box_proposal"]["AR%s@%d" % (suffix, limit)] = stats["ar"].item()
        log.info(res)
        check_expected_results(res, expected_results, expected_results_sigma_tol)
        if output_folder:
            torch.save(res, os.path.join(output_folder, "box_proposals.pth"))
        return None

    iou_types = tuple(iou_types)
    if iou_types != ("bbox",):
        raise NotImplementedError("iou_types %r: only ('bbox',) is scored here (no masks, no keypoints)" % (iou_types,))
    log.info("Preparing bbox results")
    records = prepare_for_coco_detection(predictions, dataset)
    if output_folder:
        with open(os.path.join(output_folder, "bbox.json"), "w") as f:
            json.dump(records, f)
    log.info("Evaluating predictions")
    together, per_category = box_ap.box_ap(records, dataset)
    results = COCOResults("bbox")
    for json_id, values in per_category.items():
        results.update("bbox", values, category_id=json_id)
    results.update("bbox", together)
    log.info(results)
    check_expected_results(results, expected_results, expected_results_sigma_tol)
    if output_folder:
        torch.save(results, os.path.join(output_folder, "coco_results.pth"))
    return results, {"bbox": records}


def evaluate_box_proposals(predictions, dataset, thresholds=None, area="all", limit=None):
    """Proposal recall as the reference computes it (its coco_eval.py:200-313): per image the proposals, best
    `objectness` first and cut to `limit`, against the non-crowd ground truth whose `area` lies in the range; the ground
    truth covered best by any remaining proposal is recorded with that IoU ("+1" convention) and both leave, until either
    side runs out.  Recall at each threshold = share of all in-range ground truths recorded with at least that IoU; `ar`
    is the mean over the thresholds (0.5 : 0.05 : 0.95 when none are given).  Ground truth: dataset.anns_of / dataset.ids."""
    if area not in PROPOSAL_AREAS:
        raise AssertionError("Unknown area range: {}".format(area))
    lo, hi = PROPOSAL_AREAS[area]
    covered, num_pos = [], 0
    for index, proposals in enumerate(predictions):
        info = dataset.get_img_info(index)
        size = (info["width"], info["height"])
        proposals = proposals.resize(size)
        proposals = proposals[proposals.get_field("objectness").sort(descending=True)[1]]
        anno = [a for a in dataset.anns_of.get(dataset.id_to_img_map[index], ()) if a.get("iscrowd", 0) == 0]
        if not anno:
            continue
        gt = BoxList(torch.as_tensor([a["bbox"] for a in anno]).reshape(-1, 4), size, mode="xywh").convert("xyxy")
        gt_area = torch.as_tensor([a["area"] for a in anno])
        gt = gt[(gt_area >= lo) & (gt_area <= hi)]
        num_pos += len(gt)
        if len(gt) == 0 or len(proposals) == 0:
            continue
        if limit is not None and len(proposals) > limit:
            proposals = proposals[:limit]
        overlaps = boxlist_iou(proposals, gt)
        best = torch.zeros(len(gt))
        for j in range(min(len(proposals), len(gt))):
            per_gt, which_proposal = overlaps.max(dim=0)
            value, g = per_gt.max(dim=0)
            assert value >= 0
            best[j] = value
            overlaps[which_proposal[g], :] = -1
            overlaps[:, g] = -1
        covered.append(best)
    covered = torch.sort(torch.cat(covered, dim=0) if covered else torch.zeros(0))[0]
    if thresholds is None:
        thresholds = torch.arange(0.5, 0.95 + 1e-5, 0.05, dtype=torch.float32)
    recalls = torch.zeros_like(thresholds)
    for i, t in enumerate(thresholds):
        recalls[i] = (covered >= t).float().sum() / float(num_pos)
    return {"ar": recalls.mean(), "recalls": recalls, "thresholds": thresholds, "gt_overlaps": covered,
            "num_pos": num_pos}


class COCOResults(object):
    """results[iou_type]: metric -> value, -1 until updated; for "bbox" also json category id -> {metric: value} (the
    reference's per-category entries, its coco_eval.py:378-385).  Values are plain numbers."""

    METRICS = {
        "bbox": ["AP", "AP50", "AP75", "APs", "APm", "APl"],
        "segm": ["AP", "AP50", "AP75", "APs", "APm", "APl"],
        "box_proposal": ["AR@100", "ARs@100", "ARm@100", "ARl@100", "AR@1000", "ARs@1000", "ARm@1000", "ARl@1000"],
        "keypoints": ["AP", "AP50", "AP75", "APm", "APl"],
    }

    def __init__(self, *iou_types):
        assert all(t in COCOResults.METRICS for t in iou_types), iou_types
        self.results = collections.OrderedDict(
            (t, collections.OrderedDict((metric, -1) for metric in COCOResults.METRICS[t])) for t in iou_types)

    def update(self, iou_type, values, category_id=None):
        """values: metric -> number; with `category_id` they become that category's entry instead of the overall one"""
        if values is None:
            return
        res = self.results[iou_type]
        if category_id is not None:
            res[category_id] = {metric: values[metric] for metric in COCOResults.METRICS[iou_type]}
        else:
            for metric in COCOResults.METRICS[iou_type]:
                res[metric] = values[metric]

    def table(self, names=None):
        """the bbox numbers as text: one line for all categories, one per category (`names`: json id -> label)"""
        res = self.results["bbox"]
        metrics = COCOResults.METRICS["bbox"]
        lines = ["%-16s" % "category" + "".join("%8s" % m for m in metrics),
                 "%-16s" % "all" + "".join("%8.3f" % res[m] for m in metrics)]
        for key, values in res.items():
            if isinstance(values, dict):
                label = str((names or {}).get(key, key))
                lines.append("%-16s" % label[:16] + "".join("%8.3f" % values[m] for m in metrics))
        return "\n".join(lines)

    def __repr__(self):
        return repr(self.results)


def check_expected_results(results, expected_results, sigma_tol):
    """each (task, metric, (mean, std)) must lie strictly inside mean +- sigma_tol * std; logs PASS / FAIL, never raises"""
    if not expected_results:
        return
    log = logging.getLogger("maskrcnn_benchmark.inference")
    for task, metric, (mean, std) in expected_results:
        actual = results.results[task][metric]
        lo, hi = mean - sigma_tol * std, mean + sigma_tol * std
        text = ("{} > {} sanity check (actual vs. expected): {:.3f} vs. mean={:.4f}, std={:.4}, range=({:.4f}, {:.4f})"
                .format(task, metric, actual, mean, std, lo, hi))
        if lo < actual < hi:
            log.info("PASS: " + text)
        else:
            log.error("FAIL: " + text)
