"""Error breakdown of detections: why one model's AP differs from another's.

The DA Faster R-CNN papers split the top-ranked detections into correct, mis-localised and background; TIDE (Bolya et al.,
2020) splits every false positive into classification, localisation, both, duplicate and background errors, adds the missed
ground truths, and gives for each kind the AP that fixing it alone would return.  The rule here is this project's own
statement of that breakdown on top of the PASCAL VOC matching rule (voc/voc_eval.py): it is pinned to the plain loop
evaluator of tests/_error_cases.py, not to the `tidecv` package.

Three stages, as in voc/voc_eval.py.  `pack` turns the per-image BoxLists into flat arrays with one offset pair per IMAGE,
detections in rank order (numpy sorting, nothing per detection in Python).  `match` uploads them once and gives every
detection its kind in ONE launch (`_C.error_match`, csrc/error_match.hip: one workgroup per image, all classes at once) —
there is no host matcher: without a HIP device it raises.  `summarise` is torch float64 / int64 on whatever device the flags
live on: counts, the confusion table, AP through the VOC scorer's own `class_grid` / `average_precision` (so `ap` is the VOC
scorer's, bit for bit), and the dAP of every fix."""
import collections
import json
import logging
import os

import numpy as np
import torch

from . import pairs
from .voc import voc_eval

TP, IGNORED, CLS, LOC, BOTH, DUPE, BKG = range(7)                                 # det_kind
KIND_NAMES = ("TP", "Ign", "Cls", "Loc", "Both", "Dupe", "Bkg")
DETECTED, DIFFICULT, COVERED, MISSED = range(4)                                    # gt_state
FIXES = ("Cls", "Loc", "Both", "Dupe", "Bkg", "Miss", "FP", "FN")
# one fixed colour per kind (RGB), in det_kind order, and an eighth for a missed ground truth: tools/draw_detections.py --errors
KIND_COLORS = ((40, 170, 60), (150, 150, 150), (230, 60, 200), (40, 110, 240), (140, 70, 200), (240, 150, 30), (220, 40, 40))
MISSED_COLOR = (250, 230, 40)

PackedImages = collections.namedtuple("PackedImages", [
    "n_class",        # K = largest label that occurs + 1 (0: no label occurs)
    "present",        # bool [K]: the label occurs among the detections or the ground truths
    "det_off",        # int32 [images + 1]: image i's detections, best first (stable: equal scores keep the record order)
    "gt_off",         # int32 [images + 1]: image i's ground truths, annotation order
    "det_box",        # float32 [Nd, 4] xyxy
    "det_score",      # float64 [Nd] (the float32 scores, widened)
    "det_label",      # int64 [Nd]
    "gt_box",         # float32 [Ng, 4] xyxy
    "gt_label",       # int64 [Ng]
    "gt_difficult",   # uint8 [Ng]
    "det_order",      # int64 [Nd]: packed position -> position in the concatenated records (packed = records[det_order])
    "det_restore",    # int64 [Nd]: its inverse (records = packed[det_restore])
])

Outputs = collections.namedtuple("Outputs", ["det_kind", "det_gt", "iou_same", "iou_other", "det_fix", "gt_state", "gt_det"])


def _offsets(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.int32)


def pack(pred_boxlists, gt_boxlists):
    """pred_boxlists: one BoxList per image with `labels` and `scores`; gt_boxlists: the same images' ground truth with
    `labels` and `difficult`.  Refused (ValueError): non-finite coordinates or scores, negative labels, boxes with x2 < x1 or
    y2 < y1 — so no IoU can be NaN."""
    if len(pred_boxlists) != len(gt_boxlists):
        raise AssertionError("Length of gt and pred lists need to be same.")
    det_box, gt_box = voc_eval._boxes(pred_boxlists), voc_eval._boxes(gt_boxlists)
    score = voc_eval._field(pred_boxlists, "scores", np.float32).astype(np.float64)
    label = voc_eval._field(pred_boxlists, "labels", np.int64)
    glabel = voc_eval._field(gt_boxlists, "labels", np.int64)
    difficult = (voc_eval._field(gt_boxlists, "difficult", np.int64) != 0).astype(np.uint8)
    if not (np.isfinite(det_box).all() and np.isfinite(gt_box).all()):
        raise ValueError("non-finite box coordinates cannot be scored")
    if not np.isfinite(score).all():
        raise ValueError("non-finite detection scores cannot be scored")
    if (label < 0).any() or (glabel < 0).any():
        raise ValueError("class labels must not be negative")
    for boxes in (det_box, gt_box):
        if (boxes[:, 2] < boxes[:, 0]).any() or (boxes[:, 3] < boxes[:, 1]).any():
            raise ValueError("boxes with x2 < x1 or y2 < y1 cannot be scored")
    counts = [len(b) for b in pred_boxlists]
    img = np.repeat(np.arange(len(pred_boxlists), dtype=np.int64), counts)
    K = int(max(label.max() if len(label) else -1, glabel.max() if len(glabel) else -1)) + 1
    present = np.zeros(K, dtype=bool)
    present[label] = True
    present[glabel] = True
    order = np.lexsort((-score, img)).astype(np.int64)          # stable: image, then descending score, then record order
    restore = np.empty_like(order)
    restore[order] = np.arange(len(order), dtype=np.int64)
    return PackedImages(n_class=K, present=present, det_off=_offsets(counts), gt_off=_offsets([len(b) for b in gt_boxlists]),
                        det_box=np.ascontiguousarray(det_box[order]), det_score=score[order], det_label=label[order],
                        gt_box=gt_box, gt_label=glabel, gt_difficult=difficult, det_order=order, det_restore=restore)


def match(packed, pos_thresh=0.5, bg_thresh=0.1, device=None):
    """-> Outputs on the device (see `_C.error_match`), one launch"""
    from ... import _C

    device = pairs.match_device(device, "error matching runs on the HIP device (csrc/error_match.hip): there is no CPU path")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)      # noqa: E731
    return Outputs(*_C.error_match(up(packed.det_box), up(packed.det_label.astype(np.int32)), up(packed.gt_box),
                                   up(packed.gt_label.astype(np.int32)), up(packed.gt_difficult), packed.det_off, packed.gt_off,
                                   float(pos_thresh), float(bg_thresh)))


def _ap(packed, grid, flags, n_pos, use_07_metric):
    """flags int8 [Nd] in {-1, 0, 1} and n_pos int64 [K] -> (AP float64 numpy [K], nan for a class that is absent or has no
    positives; their mean).  The operations, and the [1, K, L] shapes, are voc_eval.accumulate's and eval_detection_voc's."""
    where, counts, L = grid
    K = packed.n_class
    pad = torch.full((1, 1), -1, dtype=torch.int8, device=flags.device)
    m = torch.cat([flags[None], pad], 1)[:, where].reshape(1, K, L)
    tp = (m == 1).cumsum(-1).to(torch.float64)
    fp = (m == 0).cumsum(-1).to(torch.float64)
    prec = tp / (fp + tp)
    rec = tp / n_pos.clamp(min=1).to(torch.float64)[None, :, None]
    ap = voc_eval.average_precision(prec, rec, counts, use_07_metric).cpu().numpy()[0]
    ap[~(packed.present & (n_pos.cpu().numpy() > 0))] = np.nan
    return ap, voc_eval._nanmean(ap)


def summarise(packed, outputs, use_07_metric=False):
    """packed: `pack`'s; outputs: `match`'s seven tensors (any device; the CPU tests feed hand-made ones) -> dict, see
    DESIGN.md 3k.  Counts are int64 tensors, AP figures float64 numpy / floats."""
    out = Outputs(*outputs)
    dev = out.det_kind.device
    K = packed.n_class
    kind, fix = out.det_kind.to(torch.int64), out.det_fix.to(torch.int64)
    det_gt, state = out.det_gt.to(torch.int64), out.gt_state.to(torch.int64)
    label = torch.from_numpy(packed.det_label).to(dev)
    glabel = torch.from_numpy(packed.gt_label).to(dev)

    def per_class(labels, minlength=K):
        return torch.bincount(labels, minlength=minlength)[:minlength]

    counts = per_class(label * 7 + kind, K * 7).reshape(K, 7)
    missed, covered = per_class(glabel[state == MISSED]), per_class(glabel[state == COVERED])
    detected = per_class(glabel[state == DETECTED])
    n_pos = per_class(glabel[state != DIFFICULT])
    # the label of the defining ground truth (K, the background column, where there is none)
    target = torch.where(det_gt >= 0, glabel[det_gt.clamp(min=0)] if len(glabel) else torch.full_like(det_gt, K),
                         torch.full_like(det_gt, K))
    counted = kind != IGNORED
    confusion = per_class(label[counted] * (K + 1) + target[counted], K * (K + 1)).reshape(K, K + 1)

    base = torch.where(kind == TP, 1, torch.where(kind == IGNORED, -1, 0)).to(torch.int8)
    dropped = torch.full_like(base, -1)
    grid = pairs.class_grid(packed.det_score, packed.det_label, K, dev)
    ap, mean = _ap(packed, grid, base, n_pos, use_07_metric)

    def fixed(which):
        """flags with the detections of one kind fixed: winners of the fix claim become TP, the rest are dropped"""
        won = torch.where(fix == 1, torch.ones_like(base), dropped)
        return torch.where(kind == which, won, base)

    moved = torch.where((kind == CLS) & (fix == 1), target, label).cpu().numpy()
    scenarios = {
        "Cls": (pairs.class_grid(packed.det_score, moved, K, dev), fixed(CLS), n_pos),
        "Loc": (grid, fixed(LOC), n_pos),
        "Both": (grid, torch.where(kind == BOTH, dropped, base), n_pos),
        "Dupe": (grid, torch.where(kind == DUPE, dropped, base), n_pos),
        "Bkg": (grid, torch.where(kind == BKG, dropped, base), n_pos),
        "Miss": (grid, base, n_pos - missed),
        "FP": (grid, torch.where(base == 0, dropped, base), n_pos),
        "FN": (grid, base, detected),
    }
    dap, dap_by_class = {}, {}
    for name in FIXES:
        ap_fix, mean_fix = _ap(packed, *scenarios[name], use_07_metric)
        dap[name] = mean_fix - mean
        dap_by_class[name] = ap_fix - ap

    # the n_pos[k] best-ranked non-ignored detections of class k: shares of TP / Loc / everything else
    where, _, L = grid
    k_grid = torch.cat([kind, torch.full((1,), IGNORED, dtype=torch.int64, device=dev)])[where].reshape(K, L)
    live = k_grid != IGNORED
    taken = live & (live.cumsum(-1) <= n_pos[:, None])
    total = taken.sum(-1).to(torch.float64)
    right, loc = (taken & (k_grid == TP)).sum(-1), (taken & (k_grid == LOC)).sum(-1)
    top = torch.stack([right, loc, taken.sum(-1) - right - loc], 1).to(torch.float64) / total[:, None]     # nan: none taken
    return {"counts": counts, "missed": missed, "covered": covered, "n_pos": n_pos, "confusion": confusion, "ap": ap,
            "map": mean, "dap": dap, "dap_by_class": dap_by_class, "top_ranked": top}


def analyse(pred_boxlists, gt_boxlists, pos_thresh=0.5, bg_thresh=0.1, use_07_metric=False, device=None):
    """pack, match, summarise -> (packed, outputs, summary)"""
    packed = pack(pred_boxlists, gt_boxlists)
    outputs = match(packed, pos_thresh, bg_thresh, device)
    return packed, outputs, summarise(packed, outputs, use_07_metric)


def per_image(packed, outputs):
    """-> per image (det_kind in RECORD order, gt_state), numpy: what a drawing of that image needs"""
    kind = outputs.det_kind.cpu().numpy()[packed.det_restore]
    state = outputs.gt_state.cpu().numpy()
    return [(kind[a:b], state[c:d]) for a, b, c, d in zip(packed.det_off[:-1], packed.det_off[1:], packed.gt_off[:-1],
                                                           packed.gt_off[1:])]


_COLUMNS = ("TP", "Ign", "Cls", "Loc", "Both", "Dupe", "Bkg", "missed", "AP") + tuple("d" + f for f in FIXES)


def table(summary, names):
    """one row per class that occurs (label 0, the background, left out) plus "all"; names: label -> class name"""
    counts, missed = summary["counts"].cpu().numpy(), summary["missed"].cpu().numpy()
    lines = ["{:<16}".format("class") + "".join("{:>8}".format(c) for c in _COLUMNS)]

    def row(name, kinds, miss, ap, daps):
        cells = ["{:>8d}".format(int(v)) for v in kinds] + ["{:>8d}".format(int(miss)), "{:>8.4f}".format(ap)]
        return "{:<16}".format(name[:16]) + "".join(cells) + "".join("{:>+8.4f}".format(v) for v in daps)

    for k in range(1, len(counts)):
        if counts[k].sum() == 0 and summary["n_pos"][k] == 0 and missed[k] == 0:
            continue
        lines.append(row(names(k), counts[k], missed[k], summary["ap"][k], [summary["dap_by_class"][f][k] for f in FIXES]))
    lines.append(row("all", counts[1:].sum(0), missed[1:].sum(), summary["map"], [summary["dap"][f] for f in FIXES]))
    return "\n".join(lines) + "\n"


def _plain(value):
    """tensors, arrays and floats -> what json takes (nan -> None)"""
    if isinstance(value, dict):
        return {k: _plain(v) for k, v in value.items()}
    if isinstance(value, torch.Tensor):
        value = value.cpu().numpy()
    if isinstance(value, np.ndarray):
        return [_plain(v) for v in value.tolist()]
    if isinstance(value, (list, tuple)):
        return [_plain(v) for v in value]
    if isinstance(value, float):
        return None if value != value else value
    return value


def do_error_analysis(dataset, predictions, output_folder, logger=None, pos_thresh=0.5, bg_thresh=0.1, use_07_metric=True):
    """`predictions`: one BoxList per image of `dataset`; ground truth and sizes as in `do_voc_evaluation` (an image without
    predictions is left out together with its ground truth).  Logs the table and, with `output_folder`, writes errors.txt
    and errors.json.  -> the summary"""
    logger = logger or logging.getLogger("maskrcnn_benchmark.inference")
    if isinstance(dataset, torch.utils.data.ConcatDataset):
        dataset = voc_eval._ConcatView(dataset)
    pred_boxlists, gt_boxlists = [], []
    for image_id, prediction in enumerate(predictions):
        if len(prediction) == 0:
            continue
        info = dataset.get_img_info(image_id)
        pred_boxlists.append(prediction.resize((info["width"], info["height"])))
        gt_boxlists.append(dataset.get_groundtruth(image_id))
    _, _, summary = analyse(pred_boxlists, gt_boxlists, pos_thresh, bg_thresh, use_07_metric)
    text = "error breakdown at IoU {:g} (background below {:g}), {} metric\n".format(
        pos_thresh, bg_thresh, "11-point" if use_07_metric else "area") + table(
            summary, lambda k: str(dataset.map_class_id_to_class_name(k)).strip())
    logger.info(text)
    if output_folder:
        with open(os.path.join(output_folder, "errors.txt"), "w") as fid:
            fid.write(text)
        with open(os.path.join(output_folder, "errors.json"), "w") as fid:
            json.dump(_plain(dict(summary, pos_thresh=pos_thresh, bg_thresh=bg_thresh, use_07_metric=bool(use_07_metric),
                                  kinds=list(KIND_NAMES))), fid, indent=1, sort_keys=True)
    return summary
