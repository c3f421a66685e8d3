#!/usr/bin/env python
"""Time of COCO box AP scoring at the Cityscapes-val size: packing (host, numpy), the match launch (csrc/coco_match.hip, with
its uploads, ending in a device synchronise) and the accumulation (torch float64 on the device, ending in the host read of
the numbers), next to a plain Python / numpy loop evaluator over the same records — the loop of tests/test_coco_eval.py,
carried here so that the probe stands alone.

Data: seeded and synthetic.  --images 500 images of 2048 x 1024, 8 categories with Cityscapes-like frequencies, about 30 ground
truths per image (a few of them crowd), 100 detections per image clustered around them with float32 coordinates and scores.

Everything runs in one process on one device after a warm-up of every stage.  A window is one run of the loop and --reps
runs of the device path, in alternating order from window to window; per stage the host wall time (perf_counter; each
device stage ends in a synchronise or a host read), reported as median and range over --rounds windows.  Before anything
is timed the device path's flags are compared with the loop's for equality and the numbers within 1e-9."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from da_detect_amd.data.evaluation.coco import box_ap  # noqa: E402

W, H = 2048, 1024
FREQ = np.array([.34, .04, .51, .01, .01, .005, .015, .07])     # person rider car truck bus train motorcycle bicycle


class SyntheticSet(object):
    def __init__(self, images, seed):
        rng = np.random.default_rng(seed)
        self.ids = list(range(1000, 1000 + images))
        self.id_to_img_map = dict(enumerate(self.ids))
        self.contiguous_category_id_to_json_id = {k + 1: 24 + k for k in range(8)}
        self.anns_of, self.records = {}, []
        for image_id in self.ids:
            n = int(rng.integers(20, 41))
            side = np.exp(rng.uniform(np.log(10), np.log(400), n))
            wh = np.stack([side, side * rng.uniform(.5, 2.5, n)], 1)
            xy = rng.uniform([0, 0], [W - 10, H - 10], (n, 2))
            cat = rng.choice(8, n, p=FREQ / FREQ.sum())
            crowd = rng.uniform(0, 1, n) < .05
            self.anns_of[image_id] = [
                {"image_id": image_id, "category_id": 24 + int(cat[j]), "bbox": [float(v) for v in (*xy[j], *wh[j])],
                 "area": float(wh[j, 0] * wh[j, 1] * rng.uniform(.5, .9)), "iscrowd": int(crowd[j])} for j in range(n)]
            for _ in range(100):
                j = int(rng.integers(n))
                s = rng.choice([.03, .1, .3])
                box = np.concatenate([xy[j] + wh[j] * rng.normal(0, s, 2), wh[j] * (1 + rng.normal(0, s, 2)).clip(.1)])
                c = int(cat[j]) if rng.uniform() < .9 else int(rng.integers(8))
                self.records.append({"image_id": image_id, "category_id": 24 + c,
                                     "bbox": [float(np.float32(v)) for v in box],
                                     "score": float(np.float32(rng.uniform(.05, 1)))})


# ---- the plain loop evaluator (tests/test_coco_eval.py) --------------------------------------------------------------------------
def _loop_iou(d, g, crowd):
    dx, dy, dw, dh = (float(v) for v in d)
    gx, gy, gw, gh = (float(v) for v in g)
    w = min(dx + dw, gx + gw) - max(dx, gx)
    h = min(dy + dh, gy + gh) - max(dy, gy)
    i = max(w, 0.0) * max(h, 0.0)
    da = dw * dh
    ga = gw * gh
    u = da if crowd else (da + ga) - i
    return i / u if i > 0.0 else 0.0


def loop_box_ap(records, dataset):
    """-> dict(flags {(image position, category position): dict(matched [T][A][D], ignored [T][A][D], npig [A])},
    precision [T, R, K, A], stats [6], per_category {json id: [6]})"""
    thrs = np.linspace(.5, .95, 10)
    recs = np.linspace(0, 1, 101)
    areas = [[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]
    image_ids = list(dataset.ids)
    to_json = dataset.contiguous_category_id_to_json_id
    cat_ids = [to_json[c] for c in sorted(to_json)]
    T, R, K, A = len(thrs), len(recs), len(cat_ids), len(areas)

    dts, gts = {}, {}
    for r in records:
        dts.setdefault((r["image_id"], r["category_id"]), []).append(r)
    for image_id in image_ids:
        for a in dataset.anns_of.get(image_id, []):
            gts.setdefault((image_id, a["category_id"]), []).append(a)

    # per (image, category)
    flags = {}
    for ii, image_id in enumerate(image_ids):
        for kk, cat_id in enumerate(cat_ids):
            d = dts.get((image_id, cat_id), [])
            g = gts.get((image_id, cat_id), [])
            if not d and not g:
                continue
            order = sorted(range(len(d)), key=lambda i: -d[i]["score"])       # sorted() is stable
            d = [d[i] for i in order][:100]
            crowd = [bool(x.get("iscrowd", 0)) for x in g]
            iou = [[_loop_iou(dd["bbox"], gg["bbox"], crowd[j]) for j, gg in enumerate(g)] for dd in d]
            matched = [[[0] * len(d) for _ in range(A)] for _ in range(T)]
            ignored = [[[0] * len(d) for _ in range(A)] for _ in range(T)]
            npig = [0] * A
            for ai, (lo, hi) in enumerate(areas):
                g_ign = [crowd[j] or float(x["area"]) < lo or float(x["area"]) > hi for j, x in enumerate(g)]
                npig[ai] = sum(1 for x in g_ign if not x)
                g_order = [j for j in range(len(g)) if not g_ign[j]] + [j for j in range(len(g)) if g_ign[j]]
                for ti, t in enumerate(thrs):
                    taken = [False] * len(g)
                    for di, dd in enumerate(d):
                        best = min(float(t), 1 - 1e-10)
                        m = -1
                        for j in g_order:
                            if taken[j] and not crowd[j]:
                                continue
                            if m > -1 and not g_ign[m] and g_ign[j]:
                                break
                            if iou[di][j] < best:
                                continue
                            best = iou[di][j]
                            m = j
                        if m > -1:
                            matched[ti][ai][di] = 1
                            ignored[ti][ai][di] = 1 if g_ign[m] else 0
                            if not crowd[m]:
                                taken[m] = True
                        else:
                            d_area = float(dd["bbox"][2]) * float(dd["bbox"][3])
                            ignored[ti][ai][di] = 1 if (d_area < lo or d_area > hi) else 0
            flags[(ii, kk)] = dict(matched=matched, ignored=ignored, npig=npig, scores=[float(x["score"]) for x in d])

    # per (category, area range)
    eps = float(np.spacing(1))
    precision = -np.ones((T, R, K, A))
    for kk in range(K):
        for ai in range(A):
            pairs = [flags[(ii, kk)] for ii in range(len(image_ids)) if (ii, kk) in flags]
            scores = [s for p in pairs for s in p["scores"]]
            order = sorted(range(len(scores)), key=lambda i: -scores[i])
            npig = sum(p["npig"][ai] for p in pairs)
            if npig == 0:
                continue
            for ti in range(T):
                m = [x for p in pairs for x in p["matched"][ti][ai]]
                ig = [x for p in pairs for x in p["ignored"][ti][ai]]
                tp, fp, rc, pr = 0.0, 0.0, [], []
                for i in order:
                    if ig[i]:
                        continue
                    if m[i]:
                        tp += 1.0
                    else:
                        fp += 1.0
                    rc.append(tp / npig)
                    pr.append(tp / (fp + tp + eps))
                for i in range(len(pr) - 1, 0, -1):
                    if pr[i] > pr[i - 1]:
                        pr[i - 1] = pr[i]
                for ri, r in enumerate(recs):
                    at = len(rc)
                    for i in range(len(rc)):
                        if rc[i] >= r:
                            at = i
                            break
                    precision[ti, ri, kk, ai] = pr[at] if at < len(pr) else 0.0

    def mean_valid(cells):
        total, count = 0.0, 0
        for v in cells:
            if v > -1:
                total += float(v)
                count += 1
        return total / count if count else -1.0

    def six(cat_slice):
        p = precision[:, :, cat_slice, :]
        return [mean_valid(p[:, :, :, 0].ravel()), mean_valid(p[0, :, :, 0].ravel()), mean_valid(p[5, :, :, 0].ravel()),
                mean_valid(p[:, :, :, 1].ravel()), mean_valid(p[:, :, :, 2].ravel()), mean_valid(p[:, :, :, 3].ravel())]

    return dict(flags=flags, precision=precision, stats=six(slice(None)),
                per_category={cat_ids[kk]: six(slice(kk, kk + 1)) for kk in range(K)})


def device_path(records, dataset, times=None):
    t0 = time.perf_counter()
    packed = box_ap.pack(records, dataset)
    t1 = time.perf_counter()
    matched, ignored, npig = box_ap.match(packed)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    overall, per_category = box_ap.summarize(box_ap.accumulate(packed, matched, ignored, npig))
    overall, per_category = overall.tolist(), per_category.tolist()
    t3 = time.perf_counter()
    if times is not None:
        for k, v in (("pack", t1 - t0), ("match", t2 - t1), ("accumulate", t3 - t2), ("device path", t3 - t0)):
            times.setdefault(k, []).append(v * 1e3)
    return packed, matched, ignored, npig, overall, per_category


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("coco_eval_time.py measures on the HIP device; no device found")
    data = SyntheticSet(args.images, args.seed)
    records = data.records
    print("device %s; %d images, %d detections, %d ground truths, 8 categories" % (
        torch.cuda.get_device_name(0), len(data.ids), len(records), sum(len(v) for v in data.anns_of.values())))

    # warm-up of every stage, and equality before timing
    device_path(records, data)
    packed, matched, ignored, npig, overall, per_category = device_path(records, data)
    loop = loop_box_ap(records, data)
    K = len(packed.categories)
    matched, ignored, npig = matched.cpu().numpy(), ignored.cpu().numpy(), npig.cpu().numpy()
    assert sorted(i * K + k for i, k in loop["flags"]) == packed.pair_key.tolist()
    for p, key in enumerate(packed.pair_key.tolist()):
        f = loop["flags"][(key // K, key % K)]
        lo, hi = int(packed.det_off[p]), int(packed.det_off[p + 1])
        assert np.array_equal(matched[:, :, lo:hi], np.array(f["matched"], np.uint8).reshape(10, 4, hi - lo)), key
        assert np.array_equal(ignored[:, :, lo:hi], np.array(f["ignored"], np.uint8).reshape(10, 4, hi - lo)), key
        assert npig[p].tolist() == f["npig"], key
    worst = max(abs(a - b) for a, b in zip(overall, loop["stats"]))
    worst = max([worst] + [abs(a - b) for k, json_id in enumerate(packed.categories)
                           for a, b in zip(per_category[k], loop["per_category"][json_id])])
    assert worst <= 1e-9, worst
    gts = packed.gt_off[1:] - packed.gt_off[:-1]
    dts = packed.det_off[1:] - packed.det_off[:-1]
    print("%d pairs; per pair at most %d detections x %d ground truths; flags equal, numbers within %.1e" % (
        len(packed.pair_key), int(dts.max()), int(gts.max()), worst))
    print("AP %.4f AP50 %.4f AP75 %.4f APs %.4f APm %.4f APl %.4f" % tuple(overall))

    times = {}
    for r in range(args.rounds):
        for which in (("loop", "device") if r % 2 == 0 else ("device", "loop")):
            if which == "loop":
                t0 = time.perf_counter()
                loop_box_ap(records, data)
                times.setdefault("loop evaluator", []).append((time.perf_counter() - t0) * 1e3)
            else:
                per = {}
                for _ in range(args.reps):
                    device_path(records, data, per)
                for k, v in per.items():
                    times.setdefault(k, []).append(float(np.median(v)))
    print("%-16s %14s %28s   (%d windows; device stages: median of %d runs per window)" % (
        "stage", "host ms median", "range", args.rounds, args.reps))
    for k in ("pack", "match", "accumulate", "device path", "loop evaluator"):
        v = times[k]
        print("%-16s %14.2f %13.2f .. %-12.2f" % (k, float(np.median(v)), min(v), max(v)))
    print("loop evaluator / device path: %.1fx" % (np.median(times["loop evaluator"]) / np.median(times["device path"])))


if __name__ == "__main__":
    main()
