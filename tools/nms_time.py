#!/usr/bin/env python
"""time of one NMS (mask + sweep + compaction) on 12 000 pre-ranked boxes.

  uniform   boxes spread over the image: most of them survive (50 kept per 64-box chunk)
  clustered jittered copies of a few thousand anchors-like boxes, ranked at random — what the RPN hands over during
            training: the whole list is swept and ~10 boxes per chunk are kept (2000 of 12 000)

--batch N: the batched call (dadet_nms_batch, one launch per stage for N images) against the arrangement the RPN uses for
the same N images — per-image calls alternating over two streams (modeling/rpn/inference.py) — on the training geometry
(12 000 ranked boxes per image, quota 2000, clustered boxes, a different set per image).  Both run in one process,
alternating, after a warm-up; each timed window is --reps iterations (default 1500: windows of about a second), and
the spread is the range over the --rounds windows of the same arrangement."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from da_detect_amd import _C  # noqa: E402

dev = torch.device("cuda:0")
rng = np.random.default_rng(0)
W, H = 2048, 1024


def uniform(n, side):
    xy = np.stack([rng.uniform(0, W - 2, n), rng.uniform(0, H - 2, n)], 1)
    wh = np.stack([rng.uniform(8, side, n), rng.uniform(8, side, n)], 1)
    return np.concatenate([xy, np.minimum(xy + wh, [W - 1, H - 1])], 1).astype(np.float32)


def clustered(n, centres, jitter):
    base = uniform(centres, 400)
    pick = rng.integers(0, centres, n)
    b = base[pick] + rng.normal(0, jitter, (n, 4)).astype(np.float32)
    b[:, 2:] = np.maximum(b[:, 2:], b[:, :2] + 4)
    return np.clip(b, 0, [W - 1, H - 1, W - 1, H - 1]).astype(np.float32)


ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=0)
ap.add_argument("--reps", type=int, default=1500)
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()


def batch_against_per_image(n_img, reps, rounds, n=12000, quota=2000, thresh=0.7):
    from da_detect_amd.utils.streams import other_stream

    boxes = torch.stack([torch.from_numpy(clustered(n, 1800, 6.0)) for _ in range(n_img)]).to(dev)
    counts = [n] * n_img
    main, side = torch.cuda.current_stream(dev), other_stream(dev)

    def per_image():
        side.wait_stream(main)
        out = []
        for i in range(n_img):
            if i % 2 == 1:
                with torch.cuda.stream(side):
                    out.append(_C.nms_with_count(boxes[i], None, thresh, max_keep=quota))
            else:
                out.append(_C.nms_with_count(boxes[i], None, thresh, max_keep=quota))
        for keep, cnt in out[1::2]:
            keep.record_stream(main), cnt.record_stream(main)
        main.wait_stream(side)
        return out

    def batched():
        return _C.nms_batch_with_count(boxes, counts, thresh, max_keep=quota)

    ref = per_image()
    keep, num = batched()
    torch.cuda.synchronize()
    for i, (k1, c1) in enumerate(ref):
        assert int(c1) == int(num[i]) and torch.equal(k1[: int(c1)], keep[i, : int(c1)]), "image %d differs" % i
    print("%d images x %d boxes, quota %d: kept %s (batched == per image)" % (n_img, n, quota, num.tolist()))

    def window(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / reps

    for fn in (per_image, batched):
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    times = {"per image, two streams": [], "batched": []}
    for _ in range(rounds):
        times["per image, two streams"].append(window(per_image))
        times["batched"].append(window(batched))
    for name, t in times.items():
        print("%-24s %.4f ms per %d images (mean of %d windows of %d; min %.4f max %.4f spread %.4f; window %.2f s)" % (
            name, sum(t) / len(t), n_img, len(t), reps, min(t), max(t), max(t) - min(t), sum(t) / len(t) * reps / 1e3))
    a, b = times["per image, two streams"], times["batched"]
    gain = sum(a) / len(a) - sum(b) / len(b)
    spread = max(max(a) - min(a), max(b) - min(b))
    print("batched is %.4f ms %s; spread %.4f ms -> %s" % (abs(gain), "faster" if gain > 0 else "slower", spread,
                                                          "beyond the spread" if abs(gain) > spread else "within the spread"))


if args.batch:
    batch_against_per_image(args.batch, args.reps, args.rounds)
    sys.exit(0)

cases = [("uniform side 300", uniform(12000, 300)), ("uniform side 80", uniform(12000, 80)),
         ("clustered 1800 x jitter 6", clustered(12000, 1800, 6.0)), ("clustered 1000 x jitter 10", clustered(12000, 1000, 10.0))]
for name, arr in cases:
    b = torch.from_numpy(arr).to(dev)
    for mk in (2000, -1):
        keep, cnt = _C.nms_with_count(b, None, 0.7, max_keep=mk)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(20):
            _C.nms_with_count(b, None, 0.7, max_keep=mk)
        e.record()
        torch.cuda.synchronize()
        print("%-28s max_keep %5d: kept %5d, %.3f ms per NMS" % (name, mk, int(cnt), s.elapsed_time(e) / 20))
