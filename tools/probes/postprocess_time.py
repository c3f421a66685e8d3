#!/usr/bin/env python
"""Time of the detection filter of the evaluation path: the device filter (csrc/detect_post.hip, DADET_DEVICE_POSTPROCESS=1)
with the sweep over all ranked rows (no host read) and over the candidates after one host read, against the per-class
Python loop (DADET_DEVICE_POSTPROCESS=0, the code the filter replaces, unchanged).

Shapes (C classes, R rows per image, B images): the Cityscapes evaluation case (9, 1000, 1), a batch of eight, the 81-class
head, and a merged test-time-augmentation list (9, 6000, 1).  Seeded synthetic detections: boxes around R / 8 cluster
centres (NMS removes most of the candidates), scores the softmax of seeded logits with a bias towards the background, as a
trained head gives them.

All variants run in one process on one device, alternating, after a warm-up of every variant at every shape.  A window is
--reps calls; per window the HOST wall time per call (perf_counter around the calls, ending in a device synchronise — the
loop's cost is host waits) and the DEVICE time per call (events around the window: it includes the idle gaps the host
leaves, which is what the stream experiences).  The figure reported is the median over --rounds windows, with their range.
The three variants' results are compared bit for bit before anything is timed."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from da_detect_amd import _C  # noqa: E402
from da_detect_amd.modeling.roi_heads.box_head.inference import PostProcessor  # noqa: E402
from da_detect_amd.structures.bounding_box import BoxList  # noqa: E402

W, H = 2048, 1024
SHAPES = [(9, 1000, 1), (9, 1000, 8), (81, 1000, 2), (9, 6000, 1)]
VARIANTS = [("loop", "0", 0), ("device, no host read", "1", 0), ("device, one host read", "1", 1)]


def detections(seed, R, C, device):
    rng = np.random.default_rng(seed)
    k = max(1, R // 8)
    centres = rng.uniform([60, 60], [W - 60, H - 60], (k, 2))
    sides = rng.uniform(24, 300, (k, 2))
    which = rng.integers(0, k, (R, 1)).repeat(C, 1)
    c = centres[which] + rng.normal(0, 3, (R, C, 2))
    s = sides[which] * rng.uniform(0.9, 1.1, (R, C, 2))
    boxes = np.concatenate([c - s / 2, c + s / 2], -1)
    boxes[..., 0::2] = boxes[..., 0::2].clip(0, W - 1)
    boxes[..., 1::2] = boxes[..., 1::2].clip(0, H - 1)
    logits = rng.normal(0, 2.0, (R, C))
    logits[:, 0] += 2.0
    e = np.exp(logits - logits.max(1, keepdims=True))
    scores = e / e.sum(1, keepdims=True)
    bl = BoxList(torch.from_numpy(boxes.reshape(-1, 4).astype(np.float32)).to(device), (W, H), mode="xyxy")
    bl.add_field("scores", torch.from_numpy(scores.reshape(-1).astype(np.float32)).to(device))
    return bl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("postprocess_time.py needs a HIP device: a time taken elsewhere says nothing")
    device = torch.device("cuda:0")
    pp = PostProcessor(0.05, 0.5, 100)

    def run(variant, lists, C):
        os.environ["DADET_DEVICE_POSTPROCESS"] = variant[1]
        _C.DETECT_POST_READ_COUNTS = variant[2]
        return pp.filter_batch(lists, C)

    print("%-14s %-24s %12s %22s %12s %22s %6s %6s" % ("(C, R, B)", "variant", "host ms/call", "range", "device ms",
                                                      "range", "cand", "kept"))
    for C, R, B in SHAPES:
        lists = [detections(1000 * C + 10 * R + i, R, C, device) for i in range(B)]
        cand = sum(int((b.get_field("scores").reshape(-1, C)[:, 1:] > 0.05).sum()) for b in lists)
        uncut = PostProcessor(0.05, 0.5, -1)
        os.environ["DADET_DEVICE_POSTPROCESS"] = "0"
        kept = sum(len(r) for r in uncut.filter_batch(lists, C))
        results = [run(v, lists, C) for v in VARIANTS]
        for other in results[1:]:
            for a, b in zip(results[0], other):
                assert torch.equal(a.bbox, b.bbox) and torch.equal(a.get_field("scores"), b.get_field("scores")) and \
                    torch.equal(a.get_field("labels"), b.get_field("labels")), "variants disagree at %s" % ((C, R, B),)
        for v in VARIANTS:
            for _ in range(args.warmup):
                run(v, lists, C)
        torch.cuda.synchronize()
        host = {v[0]: [] for v in VARIANTS}
        dev = {v[0]: [] for v in VARIANTS}
        reps = max(10, args.reps // (4 if C > 9 or B > 1 else 1))      # the loop at 81 classes takes ~0.1 s per call
        for _ in range(args.rounds):
            for v in VARIANTS:            # alternating: every round times every variant
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                start.record()
                for _ in range(reps):
                    run(v, lists, C)
                stop.record()
                torch.cuda.synchronize()
                host[v[0]].append((time.perf_counter() - t0) * 1e3 / reps)
                dev[v[0]].append(start.elapsed_time(stop) / reps)
        for v in VARIANTS:
            h, d = sorted(host[v[0]]), sorted(dev[v[0]])
            print("%-14s %-24s %12.3f %22s %12.3f %22s %6d %6d" % (
                (C, R, B), v[0], h[len(h) // 2], "%.3f .. %.3f" % (h[0], h[-1]), d[len(d) // 2],
                "%.3f .. %.3f" % (d[0], d[-1]), cand, kept), flush=True)


if __name__ == "__main__":
    main()
