#!/usr/bin/env python
"""Time of PASCAL VOC AP scoring at the Cityscapes-val size: packing (host, numpy), the match launch (csrc/voc_match.hip, with
its uploads, ending in a device synchronise) and accumulation + AP (torch float64 on the device, ending in the host read of
the numbers), next to a plain numpy loop of the same rule over the same BoxLists: per image and class a vectorised float32
IoU matrix, argmax, and a Python loop over the detections for the claims, then per class a sort, two cumsums and the metric —
the shape of the scorer this package restates, carried here so that the probe stands alone.

Data: seeded and synthetic.  --images 500 images of 2048 x 1024, 8 classes with Cityscapes-like frequencies, about 30 ground
truths per image (a few of them difficult), 100 detections per image clustered around them, float32 coordinates, distinct
scores.

Everything runs in one process on one device after a warm-up of every stage.  A window is one run of the loop and --reps
runs of the device path, in alternating order from window to window; per stage the host wall time (perf_counter; each
device stage ends in a synchronise or a host read), reported as median and range over --rounds windows.  Before anything
is timed the device path's curves are compared with the loop's for equality and the APs within 1e-9."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from da_detect_amd.data.evaluation.voc import voc_eval  # noqa: E402
from da_detect_amd.structures.bounding_box import BoxList  # noqa: E402

W, H = 2048, 1024
FREQ = np.array([.34, .04, .51, .01, .01, .005, .015, .07])     # person rider car truck bus train motorcycle bicycle
THRESHOLDS = [0.5]


def synthetic_set(images, seed):
    rng = np.random.default_rng(seed)
    total = images * 100
    scores = ((rng.permutation(total) + 1.0) / (total + 1)).astype(np.float32)
    assert len(np.unique(scores)) == total
    preds, gts = [], []
    for i in range(images):
        n = int(rng.integers(20, 41))
        side = np.exp(rng.uniform(np.log(10), np.log(400), n))
        wh = np.stack([side, side * rng.uniform(.5, 2.5, n)], 1)
        xy = rng.uniform([0, 0], [W - 10, H - 10], (n, 2))
        label = rng.choice(8, n, p=FREQ / FREQ.sum()) + 1
        g = BoxList(torch.from_numpy(np.concatenate([xy, xy + wh - 1], 1).astype(np.float32)), (W, H), mode="xyxy")
        g.add_field("labels", torch.from_numpy(label.astype(np.int64)))
        g.add_field("difficult", torch.from_numpy((rng.uniform(0, 1, n) < .05).astype(np.uint8)))
        j = rng.integers(0, n, 100)
        s = rng.choice([.03, .1, .3], 100)[:, None]
        dxy = xy[j] + wh[j] * rng.normal(0, 1, (100, 2)) * s
        dwh = wh[j] * (1 + rng.normal(0, 1, (100, 2)) * s).clip(.1)
        dlabel = np.where(rng.uniform(size=100) < .9, label[j], rng.integers(1, 9, 100))
        p = BoxList(torch.from_numpy(np.concatenate([dxy, dxy + dwh - 1], 1).astype(np.float32)), (W, H), mode="xyxy")
        p.add_field("labels", torch.from_numpy(dlabel.astype(np.int64)))
        p.add_field("scores", torch.from_numpy(scores[100 * i:100 * (i + 1)]))
        preds.append(p)
        gts.append(g)
    return preds, gts


# ---- the plain numpy loop of the rule ------------------------------------------------------------------------------------
def _iou_plus_one(a, b):
    one = np.float32(1)
    area_a = (a[:, 2] - a[:, 0] + one) * (a[:, 3] - a[:, 1] + one)
    area_b = (b[:, 2] - b[:, 0] + one) * (b[:, 3] - b[:, 1] + one)
    lt = np.maximum(a[:, None, :2], b[None, :, :2])
    rb = np.minimum(a[:, None, 2:], b[None, :, 2:])
    wh = np.maximum(rb - lt + one, np.float32(0))
    inter = wh[:, :, 0] * wh[:, :, 1]
    return inter / (area_a[:, None] + area_b[None, :] - inter)


def loop_voc(preds, gts, iou_thresh, use_07_metric):
    n_pos, score, match = {}, {}, {}
    for p, g in zip(preds, gts):
        pb, pl, ps = p.bbox.numpy(), p.get_field("labels").numpy(), p.get_field("scores").numpy()
        gb, gl, gd = g.bbox.numpy(), g.get_field("labels").numpy(), g.get_field("difficult").numpy().astype(bool)
        for k in np.unique(np.concatenate([pl, gl]).astype(int)):
            mine = np.flatnonzero(pl == k)
            mine = mine[np.argsort(-ps[mine].astype(np.float64), kind="stable")]
            boxes, hard = gb[gl == k], gd[gl == k]
            n_pos[k] = n_pos.get(k, 0) + int((~hard).sum())
            score.setdefault(k, []).extend(ps[mine])
            flags = match.setdefault(k, [])
            if len(mine) == 0:
                continue
            if len(boxes) == 0:
                flags.extend([0] * len(mine))
                continue
            d, b = pb[mine].copy(), boxes.copy()
            d[:, 2:] += 1
            b[:, 2:] += 1
            iou = _iou_plus_one(d, b)
            best = iou.argmax(axis=1)
            best[iou.max(axis=1) < iou_thresh] = -1
            taken = np.zeros(len(b), dtype=bool)
            for c in best:
                if c < 0:
                    flags.append(0)
                    continue
                flags.append(-1 if hard[c] else (0 if taken[c] else 1))
                taken[c] = True
    K = max(n_pos) + 1
    prec, rec, ap = [None] * K, [None] * K, np.full(K, np.nan)
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in n_pos:
            m = np.array(match[k], dtype=np.int8)[np.argsort(-np.array(score[k], dtype=np.float64), kind="stable")]
            tp, fp = np.cumsum(m == 1), np.cumsum(m == 0)
            prec[k] = tp / (fp + tp)
            if n_pos[k] == 0:
                continue
            rec[k] = tp / n_pos[k]
            pz = np.nan_to_num(prec[k])
            if use_07_metric:
                ap[k] = 0.0
                for t in np.arange(0.0, 1.1, 0.1):
                    ap[k] += (pz[rec[k] >= t].max() if (rec[k] >= t).any() else 0.0) / 11
            else:
                mpre, mrec = np.concatenate(([0.0], pz, [0.0])), np.concatenate(([0.0], rec[k], [1.0]))
                mpre = np.maximum.accumulate(mpre[::-1])[::-1]
                i = np.flatnonzero(mrec[1:] != mrec[:-1])
                ap[k] = np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])
    return prec, rec, ap


def device_path(preds, gts, use_07_metric, times=None):
    t0 = time.perf_counter()
    packed = voc_eval.pack(preds, gts)
    t1 = time.perf_counter()
    flags, n_pos, _, _ = voc_eval.match(packed, THRESHOLDS)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    curves = voc_eval.accumulate(packed, flags, n_pos)
    ap = voc_eval.average_precision(curves.prec, curves.rec, curves.count, use_07_metric).cpu().numpy()
    t3 = time.perf_counter()
    if times is not None:
        for k, v in (("pack", t1 - t0), ("match", t2 - t1), ("accumulate + AP", t3 - t2), ("device path", t3 - t0)):
            times.setdefault(k, []).append(v * 1e3)
    ap[:, ~(curves.present & (curves.n_pos > 0))] = np.nan
    return packed, curves, ap[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--area-metric", action="store_true", help="the area metric instead of the 11-point one")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("voc_eval_time.py measures on the HIP device; no device found")
    use_07 = not args.area_metric
    preds, gts = synthetic_set(args.images, args.seed)
    print("device %s; %d images, %d detections, %d ground truths, 8 classes, IoU %.2f, %s metric" % (
        torch.cuda.get_device_name(0), len(preds), sum(len(p) for p in preds), sum(len(g) for g in gts), THRESHOLDS[0],
        "11-point" if use_07 else "area"))

    # warm-up of every stage, and equality before timing
    device_path(preds, gts, use_07)
    packed, curves, got = device_path(preds, gts, use_07)
    prec, rec, want = loop_voc(preds, gts, THRESHOLDS[0], use_07)
    got_prec, got_rec = voc_eval._curve_lists(curves, 0)
    for k in range(len(prec)):
        for a, b in ((got_prec[k], prec[k]), (got_rec[k], rec[k])):
            assert (a is None) == (b is None), k
            assert a is None or np.array_equal(a, b, equal_nan=True), k
    assert np.array_equal(np.isnan(got), np.isnan(want))
    worst = float(np.nanmax(np.abs(got - want)))
    assert worst <= 1e-9, worst
    dts, ngt = packed.det_off[1:] - packed.det_off[:-1], packed.gt_off[1:] - packed.gt_off[:-1]
    print("%d pairs; per pair at most %d detections x %d ground truths; curves equal, APs within %.1e" % (
        len(packed.pair_key), int(dts.max()), int(ngt.max()), worst))
    print("mAP %.4f; AP %s" % (float(np.nanmean(got)), " ".join("%.4f" % v for v in got[1:])))

    times = {}
    for r in range(args.rounds):
        for which in (("loop", "device") if r % 2 == 0 else ("device", "loop")):
            if which == "loop":
                t0 = time.perf_counter()
                loop_voc(preds, gts, THRESHOLDS[0], use_07)
                times.setdefault("numpy loop", []).append((time.perf_counter() - t0) * 1e3)
            else:
                per = {}
                for _ in range(args.reps):
                    device_path(preds, gts, use_07, per)
                for k, v in per.items():
                    times.setdefault(k, []).append(float(np.median(v)))
    print("%-16s %14s %28s   (%d windows; device stages: median of %d runs per window)" % (
        "stage", "host ms median", "range", args.rounds, args.reps))
    for k in ("pack", "match", "accumulate + AP", "device path", "numpy loop"):
        v = times[k]
        print("%-16s %14.2f %13.2f .. %-12.2f" % (k, float(np.median(v)), min(v), max(v)))
    print("numpy loop / device path: %.1fx" % (np.median(times["numpy loop"]) / np.median(times["device path"])))


if __name__ == "__main__":
    main()
