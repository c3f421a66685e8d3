"""COCO box AP with COCO's default parameters, written from the published definition.

Three stages.  `pack` turns the detection records and the dataset's annotations into flat float64 / int32 arrays with one
offset pair per (image, category) that has at least one detection or one ground truth: numpy sorting and segment
arithmetic, nothing per detection in Python beyond reading the record fields.  `match` uploads them once and runs the
matching of every pair in ONE launch (`_C.coco_match`, csrc/coco_match.hip) — there is no host matcher in the package: without
a HIP device it raises.  `accumulate` and `summarize` are torch float64 operations, one batched sequence for all
(threshold, area, category) rows, on whatever device the match flags live on; the CPU tests feed them flags of their own."""
import collections

import numpy as np
import torch

from .. import pairs

IOU_THRESHOLDS = np.linspace(.5, .95, 10)
RECALL_THRESHOLDS = np.linspace(0, 1, 101)
AREA_RANGES = np.array([[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]], dtype=np.float64)
MAX_DETS = 100
METRICS = ("AP", "AP50", "AP75", "APs", "APm", "APl")

Packed = collections.namedtuple("Packed", [
    "categories",   # json category ids, in contiguous-id order [K]
    "pair_key",     # image position * K + category position, ascending [P]
    "det_off",      # int32 [P + 1]: pair p's detections, best first, at most MAX_DETS
    "gt_off",       # int32 [P + 1]: pair p's ground truths, annotation order
    "det_box",      # float64 [Nd, 4] xywh
    "det_score",    # float64 [Nd]
    "det_cat",      # int64 [Nd] category position
    "gt_box",       # float64 [Ng, 4] xywh
    "gt_area",      # float64 [Ng] the annotation's `area`
    "gt_crowd",     # int32 [Ng]
])


def pack(records, dataset):
    """records: what engine.inference.prepare_for_coco_detection emits; dataset: `ids`, `anns_of`,
    `contiguous_category_id_to_json_id`"""
    image_pos = {image_id: i for i, image_id in enumerate(dataset.ids)}
    to_json = dataset.contiguous_category_id_to_json_id
    categories = [to_json[c] for c in sorted(to_json)]
    cat_pos = {json_id: k for k, json_id in enumerate(categories)}
    K = max(len(categories), 1)

    n = len(records)
    try:
        img = np.fromiter((image_pos[r["image_id"]] for r in records), dtype=np.int64, count=n)
        cat = np.fromiter((cat_pos[r["category_id"]] for r in records), dtype=np.int64, count=n)
    except KeyError as e:
        raise ValueError("a detection names image or category id %s, which the dataset does not have" % e)
    score = np.fromiter((r["score"] for r in records), dtype=np.float64, count=n)
    box = np.array([r["bbox"] for r in records], dtype=np.float64).reshape(-1, 4)

    anns = [(i, a) for i, image_id in enumerate(dataset.ids) for a in dataset.anns_of.get(image_id, ())
            if a["category_id"] in cat_pos]
    gkey = np.array([i * K + cat_pos[a["category_id"]] for i, a in anns], dtype=np.int64)
    gt_box = np.array([a["bbox"] for _, a in anns], dtype=np.float64).reshape(-1, 4)
    gt_area = np.array([a["area"] for _, a in anns], dtype=np.float64)
    gt_crowd = np.array([a.get("iscrowd", 0) for _, a in anns], dtype=np.int32)

    order, gorder, pair_key, det_off, gt_off = pairs.pair_tables(img * K + cat, score, gkey, cut=MAX_DETS)
    return Packed(categories=categories, pair_key=pair_key, det_off=det_off, gt_off=gt_off,
                  det_box=np.ascontiguousarray(box[order]), det_score=score[order], det_cat=cat[order],
                  gt_box=np.ascontiguousarray(gt_box[gorder]), gt_area=gt_area[gorder], gt_crowd=gt_crowd[gorder])


def match(packed, device=None):
    """-> (matched uint8 [T, A, Nd], ignored uint8 [T, A, Nd], npig int32 [P, A]) on the device, one launch"""
    from .... import _C

    device = pairs.match_device(device, "box AP matching runs on the HIP device (csrc/coco_match.hip): there is no CPU path")
    up = lambda a: torch.from_numpy(a).to(device)      # noqa: E731
    return _C.coco_match(up(packed.det_box), up(packed.gt_box), up(packed.gt_area), up(packed.gt_crowd), packed.det_off,
                         packed.gt_off, IOU_THRESHOLDS, AREA_RANGES)


def accumulate(packed, matched, ignored, npig):
    """precision at the recall thresholds, float64 [T, R, K, A] on the flags' device; -1 where a (category, area) has no
    non-ignored ground truth.  Every (threshold, area, category) row is a padded line of one dense tensor; an ignored
    detection (and the padding) adds to neither sum, so it repeats its left neighbour's recall and precision, which changes
    neither the right-to-left maximum nor the first index that reaches a recall threshold."""
    dev = matched.device
    T, A, n = matched.shape
    K = max(len(packed.categories), 1)
    R = len(RECALL_THRESHOLDS)
    where, _, L = pairs.class_grid(packed.det_score, packed.det_cat, K, dev)      # n = the padding column below

    pad = torch.zeros((T * A, 1), dtype=torch.uint8, device=dev)
    m = torch.cat([matched.reshape(T * A, n), pad], 1)[:, where].reshape(T, A, K, L) != 0
    counted = torch.cat([ignored.reshape(T * A, n), pad + 1], 1)[:, where].reshape(T, A, K, L) == 0
    tp = (m & counted).cumsum(-1).to(torch.float64)
    fp = (~m & counted).cumsum(-1).to(torch.float64)

    npig_cat = pairs.class_sum(packed.pair_key, K, npig, dev)                     # [K, A]
    has_gt = npig_cat.t() > 0                                                     # [A, K]
    recall = tp / npig_cat.t().clamp(min=1).to(torch.float64)[None, :, :, None]
    precision = tp / (fp + tp + float(np.spacing(1)))
    precision = precision.flip(-1).cummax(-1)[0].flip(-1)                         # non-increasing from the right
    thr = torch.from_numpy(RECALL_THRESHOLDS).to(dev).expand(T, A, K, R).contiguous()
    at = torch.searchsorted(recall.contiguous(), thr, right=False)
    q = precision.gather(-1, at.clamp(max=L - 1))
    q = torch.where(at < L, q, torch.zeros_like(q))
    q = torch.where(has_gt[None, :, :, None], q, torch.full_like(q, -1.0))
    return q.permute(0, 3, 2, 1).contiguous()                                     # [T, R, K, A]


def _mean_valid(cells, dims):
    valid = cells > -1
    count = valid.sum(dims)
    total = torch.where(valid, cells, torch.zeros_like(cells)).sum(dims)
    return torch.where(count > 0, total / count.clamp(min=1), torch.full_like(total, -1.0))


def summarize(precision):
    """precision [T, R, K, A] -> (six numbers for all categories together [6], the same per category [K, 6]); each is the
    mean over the cells > -1 of its slice, -1 for an empty slice"""
    t50 = int(np.argmin(np.abs(IOU_THRESHOLDS - .5)))
    t75 = int(np.argmin(np.abs(IOU_THRESHOLDS - .75)))
    slices = [precision[:, :, :, 0], precision[t50:t50 + 1, :, :, 0], precision[t75:t75 + 1, :, :, 0],
              precision[:, :, :, 1], precision[:, :, :, 2], precision[:, :, :, 3]]
    overall = torch.stack([_mean_valid(s, (0, 1, 2)) for s in slices])
    per_category = torch.stack([_mean_valid(s, (0, 1)) for s in slices], 1)
    return overall, per_category


def box_ap(records, dataset, device=None):
    """-> (OrderedDict metric -> value for all categories, OrderedDict json category id -> {metric: value}); the
    per-category values come from the same matching pass"""
    packed = pack(records, dataset)
    matched, ignored, npig = match(packed, device)
    overall, per_category = summarize(accumulate(packed, matched, ignored, npig))
    overall, per_category = overall.tolist(), per_category.tolist()
    together = collections.OrderedDict(zip(METRICS, overall))
    each = collections.OrderedDict((json_id, dict(zip(METRICS, per_category[k])))
                                   for k, json_id in enumerate(packed.categories))
    return together, each
