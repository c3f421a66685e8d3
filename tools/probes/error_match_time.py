#!/usr/bin/env python
"""Time of the error breakdown on a synthetic set: one `do_error_analysis` — packing (host, numpy), the match
launch (csrc/error_match.hip, with its uploads) and `summarise` (torch on the device, ending in the host read of the numbers)
— next to the plain loop evaluator the tests pin the rule to (tests/_error_cases.py: `loop_errors`, then `loop_summary`) over
the same BoxLists.

Data: seeded and synthetic.  --images 500 images of 2048 x 1024, 8 classes with Cityscapes-like frequencies, about 20 ground
truths per image (a few of them difficult), 100 detections per image clustered around them (a tenth with another label),
float32 coordinates, distinct scores.

Everything runs in one process on one device after a warm-up of every stage.  A window is one run of the loop and --reps
runs of the device path, in alternating order from window to window; host wall time (perf_counter; each device stage ends in
a synchronise or a host read), reported as median and range over --rounds windows.  Before anything is timed the launch's
seven arrays are compared with the loop's for equality and the summaries within 1e-9."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
import _error_cases as cases  # noqa: E402
from da_detect_amd.data.evaluation import errors  # noqa: E402
from da_detect_amd.structures.bounding_box import BoxList  # noqa: E402

W, H = 2048, 1024
FREQ = np.array([.34, .04, .51, .01, .01, .005, .015, .07])     # person rider car truck bus train motorcycle bicycle
NAMES = ("__background__", "person", "rider", "car", "truck", "bus", "train", "motorcycle", "bicycle")


class SyntheticSet(object):
    """what do_error_analysis touches of a dataset"""

    def __init__(self, gts):
        self.gts = gts

    def get_img_info(self, index):
        return {"width": W, "height": H}

    def get_groundtruth(self, index):
        return self.gts[index]

    def map_class_id_to_class_name(self, label):
        return NAMES[label]


def synthetic_set(images, seed):
    rng = np.random.default_rng(seed)
    total = images * 100
    scores = ((rng.permutation(total) + 1.0) / (total + 1)).astype(np.float32)
    assert len(np.unique(scores)) == total
    preds, gts = [], []
    for i in range(images):
        n = int(rng.integers(12, 29))
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
        p = BoxList(torch.from_numpy(np.concatenate([dxy, dxy + np.maximum(dwh - 1, 0)], 1).astype(np.float32)), (W, H), mode="xyxy")
        p.add_field("labels", torch.from_numpy(dlabel.astype(np.int64)))
        p.add_field("scores", torch.from_numpy(scores[100 * i:100 * (i + 1)]))
        preds.append(p)
        gts.append(g)
    return preds, gts


def device_path(preds, gts, use_07, times=None):
    t0 = time.perf_counter()
    packed = errors.pack(preds, gts)
    t1 = time.perf_counter()
    outputs = errors.match(packed, .5, .1)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    summary = errors.summarise(packed, outputs, use_07)
    counts = summary["counts"].cpu()
    t3 = time.perf_counter()
    if times is not None:
        for k, v in (("pack", t1 - t0), ("match", t2 - t1), ("summarise", t3 - t2)):
            times.setdefault(k, []).append(v * 1e3)
    return packed, outputs, summary, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--area-metric", action="store_true", help="the area metric instead of the 11-point one")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("error_match_time.py measures on the HIP device; no device found")
    use_07 = not args.area_metric
    preds, gts = synthetic_set(args.images, args.seed)
    dataset = SyntheticSet(gts)
    print("device %s; %d images, %d detections, %d ground truths, 8 classes, IoU 0.50 / 0.10, %s metric" % (
        torch.cuda.get_device_name(0), len(preds), sum(len(p) for p in preds), sum(len(g) for g in gts),
        "11-point" if use_07 else "area"), flush=True)

    # warm-up of every stage, and equality before timing
    device_path(preds, gts, use_07)
    packed, outputs, summary, _ = device_path(preds, gts, use_07)
    loop = cases.loop_errors(preds, gts)
    for name, got in zip(errors.Outputs._fields, outputs):
        got, want = got.cpu().numpy(), loop[name]
        if want.dtype == np.float32:
            got, want = got.view(np.int32), want.view(np.int32)
        assert np.array_equal(got, want), name
    want = cases.loop_summary(loop, packed.n_class, use_07)
    assert np.array_equal(summary["counts"].cpu().numpy(), want["counts"])
    worst = max(abs(summary["dap"][f] - want["dap"][f]) for f in cases.FIXES)
    worst = max(worst, abs(summary["map"] - want["map"]))
    assert worst <= 1e-9, worst
    print("the seven arrays equal the loop's; mAP and dAP within %.1e" % worst)
    print("kinds %s; mAP %.4f; dAP %s" % (dict(zip(errors.KIND_NAMES, summary["counts"].sum(0).tolist())), summary["map"],
                                          " ".join("%s %+.4f" % (f, summary["dap"][f]) for f in errors.FIXES)), flush=True)

    times = {}
    for r in range(args.rounds):
        for which in (("loop", "device") if r % 2 == 0 else ("device", "loop")):
            if which == "loop":
                t0 = time.perf_counter()
                cases.loop_summary(cases.loop_errors(preds, gts), packed.n_class, use_07)
                times.setdefault("loop evaluator", []).append((time.perf_counter() - t0) * 1e3)
            else:
                per, whole = {}, []
                for _ in range(args.reps):
                    device_path(preds, gts, use_07, per)
                    t0 = time.perf_counter()
                    errors.do_error_analysis(dataset, preds, None, use_07_metric=use_07)
                    whole.append((time.perf_counter() - t0) * 1e3)
                per["do_error_analysis"] = whole
                for k, v in per.items():
                    times.setdefault(k, []).append(float(np.median(v)))
        print("window %d done" % r, flush=True)
    print("%-18s %14s %28s   (%d windows; device stages: median of %d runs per window)" % (
        "stage", "host ms median", "range", args.rounds, args.reps))
    for k in ("pack", "match", "summarise", "do_error_analysis", "loop evaluator"):
        v = times[k]
        print("%-18s %14.2f %13.2f .. %-12.2f" % (k, float(np.median(v)), min(v), max(v)))
    print("loop evaluator / do_error_analysis: %.0fx" % (np.median(times["loop evaluator"]) / np.median(times["do_error_analysis"])))


if __name__ == "__main__":
    main()
