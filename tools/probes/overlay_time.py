#!/usr/bin/env python
"""Drawing detections at the Cityscapes size: what `render_device` costs on the device and what
`render_host` costs on the host, for the same input.

Input: 1024 x 2048 random images, each with 100 labelled records ("name 0.87" labels, outline 2) — boxes of the sizes a street
scene has (8 .. 400 pixels a side), plain and tinted (`--fill-alpha`).  Reported, all in one call on one box:

  1. `render_device` on one image and on a batch of 8 (one upload of records + glyphs + text and one launch): device time
     between two events around ONE call, the median over `--reps` calls after `--warmup` calls, next to the host time to
     issue the call (packing the records included) and the image bytes the launch would move if it touched every tile (it
     does not: a tile nothing reaches is skipped);
  2. `render_host` on the same image and records: wall time, the median over `--host-reps` calls;
  3. that both gave the same bytes.

    python tools/probes/overlay_time.py [--reps 50] [--warmup 5] [--host-reps 7] [--records 100] [--fill-alpha 0 64]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from da_detect_amd.engine import overlay  # noqa: E402

H, W = 1024, 2048
NAMES = ("person", "rider", "car", "truck", "bus", "train", "motorcycle", "bicycle")


def street_records(rng, n, fill_alpha):
    records = []
    for k in range(n):
        w, h = int(rng.integers(8, 400)), int(rng.integers(8, 400))
        x0, y0 = int(rng.integers(-20, W - 8)), int(rng.integers(-20, H - 8))
        label = int(rng.integers(1, 9))
        color = overlay.compute_colors_for_labels([label])[0]
        records.append(overlay.make_record((x0, y0, x0 + w, y0 + h), color, "%s %.2f" % (NAMES[label - 1], rng.uniform(0.7, 1.0)),
                                           thickness=2, fill_alpha=fill_alpha))
    return records


def device_ms(images, lists, reps, warmup):
    """-> (median device ms per call, median host ms per call) of render_device(images, lists); the images are drawn over
    again every call (the work does not depend on what they hold)"""
    device_times, host_times = [], []
    for k in range(warmup + reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        start.record()
        overlay.render_device(images, lists)
        stop.record()
        host = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        if k >= warmup:
            device_times.append(start.elapsed_time(stop))
            host_times.append(host)
    return statistics.median(device_times), statistics.median(host_times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=7)
    ap.add_argument("--records", type=int, default=100)
    ap.add_argument("--fill-alpha", type=int, nargs="+", default=[0, 64])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("overlay_time.py needs a HIP device: a time taken anywhere else says nothing about it")
    device = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    pixels = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(8)]
    mb = H * W * 3 * 2 / 1e6
    for alpha in args.fill_alpha:
        lists = [street_records(rng, args.records, alpha) for _ in range(8)]
        fresh = [torch.from_numpy(p).to(device) for p in pixels]
        overlay.render_device(fresh, lists)
        torch.cuda.synchronize()
        host_times, want = [], None
        for _ in range(args.host_reps):
            t0 = time.perf_counter()
            want = overlay.render_host(pixels[0], lists[0])
            host_times.append((time.perf_counter() - t0) * 1e3)
        same = np.array_equal(fresh[0].cpu().numpy(), want)
        for n in (1, 8):
            images = [torch.from_numpy(p).to(device) for p in pixels[:n]]
            dev, issue = device_ms(images, lists[:n], args.reps, args.warmup)
            print("overlay 1024x2048, %d records per image, fill alpha %3d, %d image(s) per call: device %.4f ms per call "
                  "(%.4f ms per image; upload + one launch, median of %d), host issue %.3f ms per call; %.1f MB of pixels per "
                  "image if every tile were touched" % (args.records, alpha, n, dev, dev / n, args.reps, issue, mb))
        print("overlay 1024x2048, %d records per image, fill alpha %3d: render_host %.3f ms per image (wall, median of %d); "
              "same bytes as the device: %s" % (args.records, alpha, statistics.median(host_times), args.host_reps, same))


if __name__ == "__main__":
    main()
