#!/usr/bin/env python
"""Host chain against the device input pipeline at the Cityscapes size.

Writes its own PNG files with Pillow (1024 x 2048, `--images` per domain, blocky content so that they compress and decode
like photographs rather than like noise) into a temporary directory, then reports

  1. host milliseconds per batch for 2 and for 3 domains (one image each), as the training loop spends them: fetching one
     batch of every loader plus the trainer's `images.to(device)` — host transforms + BatchCollator + upload from pageable
     memory against the `device_prep=True` loaders (decoded pixels, pinned staging, side-stream upload, one launch);
     and the PNG decode alone, which both paths pay;
  2. device time of the batched launch (`dadet_image_prepare_batch`) next to the sum of the launches it replaces (per image
     `dadet_image_resample_h` + `dadet_image_resample_v_normalize`, and the `zero_()` over the batch);
  3. with `--train N`: the `data` meter of an N-iteration `do_da_train` run (tools/train_net_da.py as a child process, with
     and without `--device-prep`; each child under its own time limit).

    python tools/probes/input_pipeline_time.py [--images 6] [--batches 12] [--train 50] [--workers 0]
"""
import argparse
import json
import os
import random
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

YAML = {2: "configs/da_faster_rcnn/e2e_da_faster_rcnn_R_50_C4_cityscapes_to_foggy_cityscapes.yaml",
        3: "configs/da_faster_rcnn/e2e_triplet_da_faster_rcnn_R_50_C4_cityscapes_to_foggy_cityscapes.yaml"}
DOMAINS = ("source", "target", "auxiliary")


def write_dataset(tmp, name, n, rng, H=1024, W=2048):
    from PIL import Image

    root = os.path.join(tmp, name)
    os.makedirs(root)
    images, annos = [], []
    for i in range(n):
        coarse = rng.integers(0, 256, (H // 16, W // 16, 3), dtype=np.uint8).repeat(16, 0).repeat(16, 1)
        fine = rng.integers(0, 8, (H, W, 3), dtype=np.uint8)
        Image.fromarray(coarse // 2 + fine * 8).save(os.path.join(root, "im%d.png" % i))
        images.append({"id": i, "file_name": "im%d.png" % i, "height": H, "width": W})
        for k in range(3):
            annos.append({"id": 3 * i + k + 1, "image_id": i, "category_id": 24 + k, "iscrowd": 0,
                          "bbox": [100 + 300 * k, 200, 250, 400], "area": 100000})
    ann = os.path.join(tmp, name + ".json")
    json.dump({"images": images, "annotations": annos,
               "categories": [{"id": 24 + k, "name": "c%d" % k} for k in range(3)]}, open(ann, "w"))
    return ann, root


def host_ms_per_batch(cfg, specs, device_prep, batches, device):
    """the loop of do_da_train without the step: one batch of every loader, joined, moved to the device"""
    from da_detect_amd.data.build import make_da_data_loaders

    random.seed(1)
    loaders = make_da_data_loaders(cfg, specs, device_prep=device_prep)
    times = []
    end = time.perf_counter()
    for parts in zip(*loaders):
        images = parts[0][0]
        for img, _, _ in parts[1:]:
            images = images + img
        images = images.to(device)
        targets = [t.to(device) for p in parts for t in p[1]]
        times.append((time.perf_counter() - end) * 1e3)
        torch.cuda.synchronize()           # (outside the timed part: the next batch starts on an idle device, as the worst case)
        del images, targets
        end = time.perf_counter()
        if len(times) >= batches:
            break
    return float(np.median(times[2:])), float(np.mean(times[2:]))


def device_times(cfg, n_images, device, reps=20):
    from da_detect_amd.data import device_prep as P

    rng = np.random.default_rng(0)
    imgs = [torch.from_numpy(rng.integers(0, 256, (1024, 2048, 3), dtype=np.uint8)).to(device) for _ in range(n_images)]
    decisions = [((600, 1200), bool(i % 2)) for i in range(n_images)]
    mean, std, bgr = cfg.INPUT.PIXEL_MEAN, cfg.INPUT.PIXEL_STD, cfg.INPUT.TO_BGR255
    batch = torch.empty((n_images, 3, 608, 1216), device=device).contiguous(memory_format=torch.channels_last)

    def batched():
        P.prepare_batch_into(imgs, decisions, mean, std, bgr, batch)

    def pairwise():
        batch.zero_()
        for i, (im, (size, flip)) in enumerate(zip(imgs, decisions)):
            P.resize_normalize_into(im, size, flip, mean, std, bgr, batch[i])

    out = {}
    for name, fn in (("batched", batched), ("pairwise", pairwise)):
        fn()
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        host = time.perf_counter()
        start.record()
        for _ in range(reps):
            fn()
        stop.record()
        host = (time.perf_counter() - host) * 1e3 / reps
        torch.cuda.synchronize()
        out[name] = (start.elapsed_time(stop) / reps, host)
    return out


def data_meter(n_domains, specs, iters, device_prep, workers):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train_net_da.py"), "--config-file", os.path.join(ROOT, YAML[n_domains])]
    for name in DOMAINS[:n_domains]:
        cmd += ["--" + name, ",".join(specs[name])]
    cmd += (["--device-prep"] if device_prep else []) + [
        "SOLVER.MAX_ITER", str(iters), "SOLVER.CHECKPOINT_PERIOD", "0", "DATALOADER.NUM_WORKERS", str(workers),
        "MODEL.WEIGHT", "", "MODEL.OUTPUT_DIR", "", "MODEL.DA_HEADS.ALIGNMENT", "False"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
    if res.returncode != 0:
        raise SystemExit("train_net_da.py failed:\n" + res.stderr[-3000:])
    lines = [ln for ln in res.stderr.splitlines() if " iter: " in ln]
    last = lines[-1]
    pick = lambda key: tuple(float(v) for v in re.search(r"\b%s: ([0-9.]+) \(([0-9.]+)\)" % key, last).groups())  # noqa: E731
    return {"iter": int(re.search(r"iter: (\d+)", last).group(1)), "data_median_avg_s": pick("data"), "time_median_avg_s": pick("time")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=6)
    ap.add_argument("--batches", type=int, default=12)
    ap.add_argument("--train", type=int, default=0, help="iterations of the do_da_train runs (0: skip them)")
    ap.add_argument("--workers", type=int, default=0)
    args = ap.parse_args()
    from PIL import Image

    from da_detect_amd.config import cfg

    device = torch.device("cuda", 0)
    with tempfile.TemporaryDirectory() as tmp:
        rng = np.random.default_rng(0)
        specs = {name: write_dataset(tmp, name, args.images, rng) for name in DOMAINS}
        for timed in (False, True):                 # (the first pass warms the page cache)
            t = time.perf_counter()
            for i in range(args.images):
                np.array(Image.open(os.path.join(specs["source"][1], "im%d.png" % i)).convert("RGB"))
        print("PNG decode (both paths pay it): %.2f ms per 1024x2048 image" % ((time.perf_counter() - t) * 1e3 / args.images))
        for n in (2, 3):
            c = cfg.clone()
            c.merge_from_file(os.path.join(ROOT, YAML[n]))
            c.merge_from_list(["SOLVER.MAX_ITER", args.batches, "DATALOADER.NUM_WORKERS", args.workers])
            sub = {k: specs[k] for k in DOMAINS[:n]}
            for device_prep in (False, True):
                med, mean = host_ms_per_batch(c, sub, device_prep, args.batches, device)
                print("%d domains, %s: host %.2f ms per batch (median; mean %.2f), %d workers"
                      % (n, "device path" if device_prep else "host chain ", med, mean, args.workers))
            for name, (dev_ms, host_ms) in device_times(c, n, device).items():
                print("%d images, %s launches: device %.3f ms, host issue %.3f ms" % (n, name, dev_ms, host_ms))
        if args.train:
            for n in (2, 3):
                sub = {k: specs[k] for k in DOMAINS[:n]}
                for device_prep in (False, True):
                    print("%d domains, do_da_train %d iterations, %s: %s" % (
                        n, args.train, "device path" if device_prep else "host chain ",
                        data_meter(n, sub, args.train, device_prep, args.workers)))


if __name__ == "__main__":
    main()
