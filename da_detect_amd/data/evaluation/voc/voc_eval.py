"""PASCAL VOC average precision (reference: data/datasets/evaluation/voc/voc_eval.py), DESIGN.md 3e.

Three stages, as in coco/box_ap.py.  `pack` turns the per-image BoxLists into flat float32 arrays with one offset pair per
(image, class) that has at least one detection or one ground truth: numpy sorting, nothing per detection in Python.  `match`
uploads them once and matches every pair, for every IoU threshold, in ONE launch (`_C.voc_match`, csrc/voc_match.hip) — there
is no host matcher in the package: without a HIP device it raises.  `accumulate` and `average_precision` are torch float64
operations, one batched sequence over a padded [T, K, L] tensor (thresholds, classes, detections of the fullest class), on
whatever device the match flags live on; the CPU tests feed them flags of their own.

Tie order.  Between equal scores the reference's order is whatever numpy's unstable `argsort()[::-1]` leaves.  Here it is
stable: image order first, then the pair's order (a pair keeps the record order of its equal scores).  With distinct scores
the two agree exactly.

Beyond the reference: `iou_thresh` may be a sequence (all thresholds come from the one launch; the result then also carries
"ap_by_iou" [T, K], and "ap" / "map" are those of the first threshold), and `do_voc_evaluation` takes `iou_thresh` and
`use_07_metric` instead of fixing them (its defaults are the reference's: 0.5 and the 11-point metric)."""
import bisect
import collections
import logging
import os

import numpy as np
import torch

from .. import pairs

Packed = collections.namedtuple("Packed", [
    "n_class",        # K = largest label that occurs + 1 (0: no label occurs)
    "present",        # bool [K]: the label occurs among the detections or the ground truths
    "pair_key",       # image position * K + label, ascending [P]
    "det_off",        # int32 [P + 1]: pair p's detections, best first (not cut: VOC has no detection limit)
    "gt_off",         # int32 [P + 1]: pair p's ground truths, annotation order
    "det_box",        # float32 [Nd, 4] xyxy
    "det_score",      # float64 [Nd] (the float32 scores, widened)
    "det_label",      # int64 [Nd]
    "gt_box",         # float32 [Ng, 4] xyxy
    "gt_difficult",   # uint8 [Ng]
])

Curves = collections.namedtuple("Curves", [
    "prec",           # float64 [T, K, L]: tp / (fp + tp), nan where both are 0; past a class's count the last value repeats
    "rec",            # float64 [T, K, L]: tp / n_pos (n_pos of 0 divides by 1; see `n_pos`)
    "count",          # int64 numpy [K]: detections of the class
    "n_pos",          # int64 numpy [K]: non-difficult ground truths of the class
    "present",        # bool numpy [K]
])


def _field(boxlists, name, dtype):
    parts = [np.asarray(b.get_field(name).detach().cpu().numpy()).reshape(-1) for b in boxlists]
    return np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype=dtype)


def _boxes(boxlists):
    parts = [b.convert("xyxy").bbox.detach().cpu().numpy().astype(np.float32).reshape(-1, 4) for b in boxlists]
    return np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros((0, 4), dtype=np.float32)


def pack(pred_boxlists, gt_boxlists):
    """pred_boxlists: one BoxList per image with `labels` and `scores`; gt_boxlists: the same images' ground truth with
    `labels` and `difficult`.  Non-finite coordinates or scores are refused."""
    if len(pred_boxlists) != len(gt_boxlists):
        raise AssertionError("Length of gt and pred lists need to be same.")
    det_box, gt_box = _boxes(pred_boxlists), _boxes(gt_boxlists)
    score = _field(pred_boxlists, "scores", np.float32).astype(np.float64)
    label = _field(pred_boxlists, "labels", np.int64)
    glabel = _field(gt_boxlists, "labels", np.int64)
    difficult = (_field(gt_boxlists, "difficult", np.int64) != 0).astype(np.uint8)
    if not (np.isfinite(det_box).all() and np.isfinite(gt_box).all()):
        raise ValueError("non-finite box coordinates cannot be scored")
    if not np.isfinite(score).all():
        raise ValueError("non-finite detection scores cannot be scored")
    if (label < 0).any() or (glabel < 0).any():
        raise ValueError("class labels must not be negative")
    img = np.repeat(np.arange(len(pred_boxlists), dtype=np.int64), [len(b) for b in pred_boxlists])
    gimg = np.repeat(np.arange(len(gt_boxlists), dtype=np.int64), [len(b) for b in gt_boxlists])

    K = int(max(label.max() if len(label) else -1, glabel.max() if len(glabel) else -1)) + 1
    present = np.zeros(K, dtype=bool)
    present[label] = True
    present[glabel] = True
    order, gorder, pair_key, det_off, gt_off = pairs.pair_tables(img * K + label, score, gimg * K + glabel)
    return Packed(n_class=K, present=present, pair_key=pair_key, det_off=det_off, gt_off=gt_off,
                  det_box=np.ascontiguousarray(det_box[order]), det_score=score[order], det_label=label[order],
                  gt_box=np.ascontiguousarray(gt_box[gorder]), gt_difficult=difficult[gorder])


def match(packed, iou_thresholds, device=None):
    """-> (match int8 [T, Nd] in {-1, 0, 1}, n_pos int32 [P], gt_index int32 [Nd], iou_max float32 [Nd]) on the device, one
    launch for all thresholds"""
    from .... import _C

    device = pairs.match_device(device, "VOC matching runs on the HIP device (csrc/voc_match.hip): there is no CPU path")
    up = lambda a: torch.from_numpy(a).to(device)      # noqa: E731
    return _C.voc_match(up(packed.det_box), up(packed.gt_box), up(packed.gt_difficult), packed.det_off, packed.gt_off,
                        [float(t) for t in iou_thresholds])


def accumulate(packed, match, n_pos):
    """match int8 [T, Nd] and n_pos int [P] in packed order -> Curves.  Per class the detections in descending score (stable:
    image order, then the pair's order); tp = cumsum(match == 1), fp = cumsum(match == 0) — a -1 (difficult) and the padding
    add to neither, so they repeat their left neighbour's values."""
    dev = match.device
    T, n = match.shape
    K = packed.n_class
    where, counts, L = pairs.class_grid(packed.det_score, packed.det_label, K, dev)     # n = the padding column below

    pad = torch.full((T, 1), -1, dtype=torch.int8, device=dev)
    m = torch.cat([match, pad], 1)[:, where].reshape(T, K, L)
    tp = (m == 1).cumsum(-1).to(torch.float64)
    fp = (m == 0).cumsum(-1).to(torch.float64)
    n_pos_class = pairs.class_sum(packed.pair_key, K, n_pos, dev)
    prec = tp / (fp + tp)
    rec = tp / n_pos_class.clamp(min=1).to(torch.float64)[None, :, None]
    return Curves(prec=prec, rec=rec, count=counts, n_pos=n_pos_class.cpu().numpy(), present=packed.present)


def average_precision(prec, rec, count, use_07_metric=False):
    """prec / rec float64 [T, K, L] (class k's curve in its first count[k] columns), count [K] -> AP float64 [T, K].
    11-point metric: for t in arange(0, 1.1, 0.1), in that order, ap += max(prec where rec >= t, else 0) / 11.  Area metric:
    sentinels (0, 0) and (1, 0), right-to-left maximum of the precision, sum of recall step x precision over the steps."""
    dev = prec.device
    T, K, L = prec.shape
    valid = (torch.arange(L, device=dev)[None, :] < torch.as_tensor(np.asarray(count), device=dev)[:, None])[None]
    p = torch.where(valid, torch.nan_to_num(prec, nan=0.0), torch.zeros_like(prec))
    if use_07_metric:
        ap = torch.zeros((T, K), dtype=torch.float64, device=dev)
        for t in np.arange(0.0, 1.1, 0.1):
            reached = valid & (rec >= float(t))
            ap = ap + torch.where(reached, p, torch.zeros_like(p)).amax(-1) / 11
        return ap
    # past its count a class repeats its last recall (0 for an empty class): steps of width 0, which add nothing
    last = rec.gather(-1, (torch.as_tensor(np.asarray(count), device=dev) - 1).clamp(min=0)[None, :, None].expand(T, K, 1))
    last = torch.where(valid[..., :1], last, torch.zeros_like(last))
    r = torch.where(valid, rec, last)
    zero, one = torch.zeros((T, K, 1), dtype=torch.float64, device=dev), torch.ones((T, K, 1), dtype=torch.float64, device=dev)
    mpre = torch.cat([zero, p, zero], -1).flip(-1).cummax(-1)[0].flip(-1)
    mrec = torch.cat([zero, r, one], -1)
    step = mrec[..., 1:] - mrec[..., :-1]
    return torch.where(step != 0, step * mpre[..., 1:], torch.zeros_like(step)).sum(-1)


def _curve_lists(curves, t):
    """the reference's (prec, rec) lists of one threshold: None for a label that never occurs, rec None without positives"""
    prec_t, rec_t = curves.prec[t].cpu().numpy(), curves.rec[t].cpu().numpy()
    prec, rec = [None] * len(curves.count), [None] * len(curves.count)
    for k in np.flatnonzero(curves.present):
        prec[k] = prec_t[k, :curves.count[k]].copy()
        if curves.n_pos[k] > 0:
            rec[k] = rec_t[k, :curves.count[k]].copy()
    return prec, rec


def _curves(pred_boxlists, gt_boxlists, thresholds):
    packed = pack(pred_boxlists, gt_boxlists)
    flags, n_pos, _, _ = match(packed, thresholds)
    return accumulate(packed, flags, n_pos)


def _thresholds(iou_thresh):
    many = isinstance(iou_thresh, (list, tuple, np.ndarray))
    return many, [float(t) for t in (iou_thresh if many else [iou_thresh])]


def calc_detection_voc_prec_rec(gt_boxlists, pred_boxlists, iou_thresh=0.5):
    """-> (prec, rec): per label a float64 array over that class's detections in descending score, or None (see
    `_curve_lists`).  With a sequence of thresholds: one such pair of lists per threshold, `([prec_t...], [rec_t...])`."""
    many, thr = _thresholds(iou_thresh)
    curves = _curves(pred_boxlists, gt_boxlists, thr)
    each = [_curve_lists(curves, t) for t in range(len(thr))]
    return ([e[0] for e in each], [e[1] for e in each]) if many else each[0]


def calc_detection_voc_ap(prec, rec, use_07_metric=False):
    """the reference's signature: lists of arrays with None holes -> float64 ndarray [len(prec)], nan at a hole"""
    K = len(prec)
    ok = np.array([prec[k] is not None and rec[k] is not None for k in range(K)], dtype=bool)
    count = np.array([len(prec[k]) if ok[k] else 0 for k in range(K)], dtype=np.int64)
    L = max(int(count.max()) if K else 0, 1)
    p, r = torch.zeros((1, K, L), dtype=torch.float64), torch.zeros((1, K, L), dtype=torch.float64)
    for k in np.flatnonzero(ok):
        p[0, k, :count[k]] = torch.as_tensor(np.asarray(prec[k], dtype=np.float64))
        r[0, k, :count[k]] = torch.as_tensor(np.asarray(rec[k], dtype=np.float64))
    ap = average_precision(p, r, count, use_07_metric)[0].numpy().copy()
    ap[~ok] = np.nan
    return ap


def _nanmean(values):
    kept = values[~np.isnan(values)]
    return float(kept.mean()) if len(kept) else float("nan")


def eval_detection_voc(pred_boxlists, gt_boxlists, iou_thresh=0.5, use_07_metric=False):
    """-> {"ap": float64 ndarray [largest label + 1], nan for a label that never occurs or has no non-difficult ground
    truth; "map": their mean over the non-nan entries}; with a sequence `iou_thresh` also "ap_by_iou" [T, K] (and "ap" /
    "map" are the first threshold's)."""
    assert len(gt_boxlists) == len(pred_boxlists), "Length of gt and pred lists need to be same."
    many, thr = _thresholds(iou_thresh)
    curves = _curves(pred_boxlists, gt_boxlists, thr)
    ap = average_precision(curves.prec, curves.rec, curves.count, use_07_metric).cpu().numpy()
    ap[:, ~(curves.present & (curves.n_pos > 0))] = np.nan
    result = {"ap": ap[0], "map": _nanmean(ap[0])}
    if many:
        result["ap_by_iou"] = ap
    return result


class _ConcatView(object):
    """a ConcatDataset of VOC-style datasets seen as one: the members do_voc_evaluation touches"""

    def __init__(self, concat):
        self.parts, self.ends = list(concat.datasets), list(concat.cumulative_sizes)
        self.get_img_info = concat.get_img_info
        self.map_class_id_to_class_name = self.parts[0].map_class_id_to_class_name
        names = [getattr(d, "CLASSES", None) for d in self.parts]
        if any(n != names[0] for n in names):
            raise ValueError("the concatenated datasets have different classes")

    def get_groundtruth(self, index):
        which = bisect.bisect_right(self.ends, index)
        return self.parts[which].get_groundtruth(index if which == 0 else index - self.ends[which - 1])


def do_voc_evaluation(dataset, predictions, output_folder, logger=None, iou_thresh=0.5, use_07_metric=True):
    """`predictions`: one BoxList per image of `dataset` (`get_img_info`, `get_groundtruth`, `map_class_id_to_class_name`).
    An image without predictions is left out together with its ground truth, as in the reference (its lines 17-27).  Logs
    and, with `output_folder`, writes result.txt: mAP, then one line per class."""
    logger = logger or logging.getLogger("maskrcnn_benchmark.inference")
    if isinstance(dataset, torch.utils.data.ConcatDataset):
        dataset = _ConcatView(dataset)
    pred_boxlists, gt_boxlists = [], []
    for image_id, prediction in enumerate(predictions):
        if len(prediction) == 0:
            continue
        info = dataset.get_img_info(image_id)
        pred_boxlists.append(prediction.resize((info["width"], info["height"])))
        gt_boxlists.append(dataset.get_groundtruth(image_id))
    result = eval_detection_voc(pred_boxlists=pred_boxlists, gt_boxlists=gt_boxlists, iou_thresh=iou_thresh,
                                use_07_metric=use_07_metric)
    result_str = "mAP: {:.4f}\n".format(result["map"])
    for i, ap in enumerate(result["ap"]):
        if i == 0:      # background
            continue
        result_str += "{:<16}: {:.4f}\n".format(dataset.map_class_id_to_class_name(i), ap)
    logger.info(result_str)
    if output_folder:
        with open(os.path.join(output_folder, "result.txt"), "w") as fid:
            fid.write(result_str)
    return result
