#!/usr/bin/env python
"""Rain synthesis at the Cityscapes size: what it costs on the device, and what the aligned triplet
loader spends on the host with an on-disk auxiliary set against `rain:MASKDIR`.

Writes its own PNG files (1024 x 2048 images as tools/probes/input_pipeline_time.py writes them, and a few rain masks) into
a temporary directory, then reports, all in one call on one box:

  1. device time of one `dadet_rain_synthesize` at 1024 x 2048 (event-timed over `--reps` calls) for a depth-2 and a depth-3
     plan, next to its host issue time;
  2. host milliseconds per batch of `make_triplet_data_loader(..., device_prep=True)` — one aligned triplet per batch plus
     the trainer's join and `.to(device)`, as the loop spends them — with the auxiliary images read from disk (three PNG
     decodes per triplet) against `rain:` (two decodes, the rainy image synthesised on the side stream), with
     `DATALOADER.NUM_WORKERS 0`, each pair twice.

    python tools/probes/rain_time.py [--images 6] [--batches 12] [--reps 20]
"""
import argparse
import os
import random
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from input_pipeline_time import YAML, write_dataset  # noqa: E402


def write_masks(folder, n, rng, H=512, W=1024):
    from PIL import Image

    os.makedirs(folder)
    for k in range(n):
        grey = np.clip((rng.random((H, W)) ** 6) * 320.0 - 8.0, 0, 255).astype(np.uint8)
        Image.fromarray(np.stack([grey] * 3, axis=2)).save(os.path.join(folder, "mask%d.png" % k))
    return folder


def device_time(device, reps):
    from da_detect_amd.data import rain

    rng = np.random.default_rng(0)
    H, W = 1024, 2048
    image = rain.upload(rng.integers(0, 256, (H, W, 3), dtype=np.uint8), device)
    mask = rain.upload(np.clip((rng.random((H, W, 3)) ** 6) * 320.0, 0, 255).astype(np.uint8), device)
    out = torch.empty_like(image)
    scratch = torch.empty(rain.scratch_bytes(H, W, 3), dtype=torch.uint8, device=device)
    for seed in (1, 21):                             # a depth-2 and a depth-3 plan
        plan = rain.draw_rain_plan(np.random.RandomState(seed), W, H)
        rain.synthesize_device(image, mask, plan, out=out, scratch=scratch)
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        host = time.perf_counter()
        start.record()
        for _ in range(reps):
            rain.synthesize_device(image, mask, plan, out=out, scratch=scratch)
        stop.record()
        host = (time.perf_counter() - host) * 1e3 / reps
        torch.cuda.synchronize()
        ops = " | ".join(",".join(op[0] for op in chain) for chain in plan.ops)
        print("synthesis 1024x2048, depth %d (%d launches; %s): device %.3f ms, host issue %.3f ms"
              % (plan.depth, plan.depth, ops, start.elapsed_time(stop) / reps, host))


def host_ms_per_batch(cfg, specs, batches, device):
    from da_detect_amd.data.build import make_triplet_data_loader

    random.seed(1)
    loader = make_triplet_data_loader(cfg, specs, device_prep=True)
    times = []
    end = time.perf_counter()
    for s_img, s_tgt, p_img, p_tgt, n_img, n_tgt, _, _, _ in loader:
        images = (s_img + p_img + n_img).to(device)
        targets = [t.to(device) for t in list(s_tgt) + list(p_tgt) + list(n_tgt)]
        times.append((time.perf_counter() - end) * 1e3)
        torch.cuda.synchronize()           # (outside the timed part: the next batch starts on an idle device)
        del images, targets
        end = time.perf_counter()
        if len(times) >= batches:
            break
    return float(np.median(times[2:])), float(np.mean(times[2:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=6)
    ap.add_argument("--batches", type=int, default=12)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    from da_detect_amd.config import cfg

    device = torch.device("cuda", 0)
    device_time(device, args.reps)
    with tempfile.TemporaryDirectory() as tmp:
        rng = np.random.default_rng(0)
        specs = {name: write_dataset(tmp, name, args.images, rng) for name in ("source", "target", "auxiliary")}
        rainy = dict(specs, auxiliary=("rain:" + write_masks(os.path.join(tmp, "masks"), 3, rng), ""))
        c = cfg.clone()
        c.merge_from_file(os.path.join(ROOT, YAML[3]))
        c.merge_from_list(["SOLVER.MAX_ITER", args.batches, "DATALOADER.NUM_WORKERS", 0])
        for rounds in range(2):                      # each pair twice, alternating: drift of the box shows as a difference
            for name, sub in (("on-disk auxiliary", specs), ("rain:MASKDIR      ", rainy)):
                med, mean = host_ms_per_batch(c, sub, args.batches, device)
                print("aligned triplet, device path, %s: host %.2f ms per batch (median; mean %.2f), 0 workers, pass %d"
                      % (name, med, mean, rounds))


if __name__ == "__main__":
    main()
