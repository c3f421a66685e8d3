"""What the COCO and the PASCAL VOC scorers (coco/box_ap.py, voc/voc_eval.py) share: the offset tables of the
(image, class) pairs on the host, the choice of the device to match on, and the padded [K, L] per-class grid their
`accumulate` gathers the match flags through."""
import numpy as np
import torch

from ..._lib import DadetError


def _offsets(sorted_keys, pairs):
    off = np.searchsorted(sorted_keys, pairs, side="left")
    return np.append(off, len(sorted_keys)).astype(np.int32)


def pair_tables(det_key, det_score, gt_key, cut=None):
    """det_key / gt_key: image position * K + class of every detection / ground truth -> (det_order, gt_order, pair_key,
    det_off, gt_off).  det_order lists a pair's detections best first, at most `cut` of them (stable: equal scores of a pair
    keep the record order); gt_order keeps the annotation order inside a pair; pair_key holds, ascending, every key with a
    detection or a ground truth, and pair p owns det_order[det_off[p]:det_off[p + 1]] and the same slice of gt_order."""
    order = np.lexsort((-det_score, det_key))
    key_sorted = det_key[order]
    if cut is not None:
        first = np.searchsorted(key_sorted, key_sorted, side="left")
        keep = np.arange(len(order)) - first < cut
        order, key_sorted = order[keep], key_sorted[keep]
    gorder = np.argsort(gt_key, kind="stable")
    gkey_sorted = gt_key[gorder]
    pairs = np.union1d(key_sorted, gkey_sorted)
    return order, gorder, pairs, _offsets(key_sorted, pairs), _offsets(gkey_sorted, pairs)


def match_device(device, no_device_message):
    """the device the matching kernel runs on: the one asked for, else the current HIP device; there is no CPU path"""
    if device is not None:
        return device
    if not torch.cuda.is_available():
        raise DadetError(no_device_message)
    return torch.device("cuda", torch.cuda.current_device())


def class_grid(score, label, K, dev):
    """score float64 [n] / label int64 [n] numpy, in packed order -> (where int64 [K, L] on dev, counts int64 numpy [K], L).
    Row k of `where` lists class k's detections in descending score (stable: ties keep the packed order, which is image order,
    then the pair's order); past the class's count it holds n, the padding column the caller appends.  L = the fullest
    class's count, at least 1."""
    n = len(score)
    counts = np.bincount(label, minlength=K).astype(np.int64)
    L = max(int(counts.max()) if K else 0, 1)
    score, label = torch.from_numpy(score).to(dev), torch.from_numpy(label).to(dev)
    by_score = torch.sort(score, descending=True, stable=True)[1]
    by_label = torch.sort(label[by_score], stable=True)[1]
    order = by_score[by_label]
    label_sorted = label[order]
    start = torch.from_numpy(np.cumsum(counts) - counts).to(dev)
    column = torch.arange(n, device=dev) - start[label_sorted]
    where = torch.full((K, L), n, dtype=torch.int64, device=dev)
    where[label_sorted, column] = order
    return where, counts, L


def class_sum(pair_key, K, per_pair, dev):
    """per_pair int [P, ...] (one row per pair) -> int64 [K, ...] on dev: the sum over the pairs of each class"""
    pair_class = torch.from_numpy(pair_key % max(K, 1)).to(dev)
    per_pair = per_pair.to(dev).to(torch.int64)
    return torch.zeros((K,) + tuple(per_pair.shape[1:]), dtype=torch.int64, device=dev).index_add_(0, pair_class, per_pair)
