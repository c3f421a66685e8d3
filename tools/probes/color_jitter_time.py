#!/usr/bin/env python
"""Colour jitter at the Cityscapes size: what it costs on the device, and what the loaders spend on
the host with the four jitters on, host chain against `--device-prep`.

Writes its own 1024 x 2048 PNG files (as tools/probes/input_pipeline_time.py writes them) into a temporary directory, then
reports, all in one call on one box and without worker processes (section 3g says why):

  1. device time per image of `dadet_color_jitter_batch` at 1024 x 2048 (event-timed over `--reps` calls, one image and a
     batch of four) for operator lists that take the apply pass alone and lists that add the sum pass, next to the bytes
     the passes move (6.3 MB read by the sum pass; 6.3 MB read and 6.3 MB written by the apply pass) and the host issue time;
  2. host milliseconds per batch of `make_da_data_loaders` with INPUT.BRIGHTNESS / CONTRAST / SATURATION / HUE set, on the
     host chain and on the device path, and the device path with the keys at their defaults, each twice in alternation.

    python tools/probes/color_jitter_time.py [--images 4] [--batches 6] [--reps 20]
"""
import argparse
import os
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from input_pipeline_time import YAML, host_ms_per_batch, write_dataset  # noqa: E402

B, C, S, H = ("brightness", 1.2), ("contrast", 0.8), ("saturation", 1.3), ("hue", 0.05)
LISTS = [("brightness", [B]), ("saturation", [S]), ("hue", [H]), ("brightness, saturation, hue", [B, S, H]),
         ("contrast", [C]), ("contrast first of four", [C, B, S, H]), ("contrast last of four", [B, S, H, C])]


def device_time(device, reps):
    from da_detect_amd import _lib
    from da_detect_amd.data.color_jitter import jitter_device

    rng = np.random.default_rng(0)
    Hh, W = 1024, 2048
    mb = Hh * W * 3 / 1e6
    images = [torch.from_numpy(rng.integers(0, 256, (Hh, W, 3), dtype=np.uint8)).to(device) for _ in range(4)]
    sums = torch.empty(_lib.JITTER_BATCH_MAX, dtype=torch.int64, device=device)
    for n in (1, 4):
        for name, ops in LISTS:
            passes = 2 if any(op == "contrast" for op, _ in ops) else 1
            jitter_device(images[:n], [ops] * n, sums)
            torch.cuda.synchronize()
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            host = time.perf_counter()
            start.record()
            for _ in range(reps):
                jitter_device(images[:n], [ops] * n, sums)
            stop.record()
            host = (time.perf_counter() - host) * 1e3 / reps
            torch.cuda.synchronize()
            ms = start.elapsed_time(stop) / reps / n
            moved = mb * (passes + 1)
            print("jitter 1024x2048, %d image(s) per call, %-28s: %d launch(es), device %.4f ms per image, %.1f MB moved -> "
                  "%.2f TB/s, host issue %.3f ms per call" % (n, name, passes, ms, moved, moved / ms / 1e3, host))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    from da_detect_amd.config import cfg

    device = torch.device("cuda", 0)
    device_time(device, args.reps)
    with tempfile.TemporaryDirectory() as tmp:
        rng = np.random.default_rng(0)
        specs = {name: write_dataset(tmp, name, args.images, rng) for name in ("source", "target")}
        plain = cfg.clone()
        plain.merge_from_file(os.path.join(ROOT, YAML[2]))
        plain.merge_from_list(["SOLVER.MAX_ITER", args.batches, "DATALOADER.NUM_WORKERS", 0])
        jitter = plain.clone()
        jitter.merge_from_list(["INPUT.BRIGHTNESS", 0.4, "INPUT.CONTRAST", 0.4, "INPUT.SATURATION", 0.4, "INPUT.HUE", 0.1])
        for rounds in range(2):                      # each twice, alternating: drift of the box shows as a difference
            for name, c, device_prep in (("four jitters, host chain ", jitter, False), ("four jitters, device path", jitter, True),
                                         ("default keys, device path", plain, True)):
                med, mean = host_ms_per_batch(c, specs, device_prep, args.batches, device)
                print("source + target loaders, %s: host %.2f ms per batch (median; mean %.2f), 0 workers, pass %d"
                      % (name, med, mean, rounds))


if __name__ == "__main__":
    main()
