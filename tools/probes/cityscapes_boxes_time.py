#!/usr/bin/env python
"""Instance boxes from id maps at the Cityscapes size: what each part of the conversion costs.

At 1024 x 2048 with about 40 synthetic instances it reports, each as the median of `--reps` runs after two warm-up runs:

  1. device time per map of `dadet_instance_boxes` (table clear + accumulation + compaction) from stream events, for one map
     and for a batch of 16;
  2. upload time per map (pinned staging buffer -> device, stream events) and the copy of the result rows back;
  3. `instance_table_host` (numpy) per map;
  4. Pillow's decode of the 16-bit PNG per map.

Then the wall time of converting a synthetic split of `--images` maps (default 200, written as PNG into a temporary
directory) with `build_annotations` on the device and on the host path, each pass twice, alternating.

    python tools/probes/cityscapes_boxes_time.py [--images 200] [--reps 15]
"""
import argparse
import ctypes
import os
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W = 1024, 2048


def synthetic_map(seed, instances=40):
    rng = np.random.RandomState(seed)
    ids = rng.choice([7, 8, 11, 21, 23], size=(H // 64, W // 64)).repeat(64, 0).repeat(64, 1).astype(np.uint16)
    yy, xx = np.mgrid[0:H, 0:W]
    for k in range(instances):
        value = int(rng.choice([24, 25, 26, 27, 28, 31, 32, 33])) * 1000 + k
        cy, cx, h, w = int(rng.randint(300, 900)), int(rng.randint(0, W)), int(rng.randint(10, 300)), int(rng.randint(6, 400))
        if k % 2:
            ids[max(cy - h // 2, 0):cy + h // 2, max(cx - w // 2, 0):cx + w // 2] = value
        else:
            ids[((yy - cy) / (h / 2.0)) ** 2 + ((xx - cx) / (w / 2.0)) ** 2 <= 1.0] = value
    return ids


def median_ms(samples):
    return float(np.median(samples))


def device_times(maps, reps, device):
    from da_detect_amd import _lib
    from da_detect_amd.data import cityscapes as cs

    n = len(maps)
    total = n * H * W
    staging = torch.empty(total, dtype=torch.int16, pin_memory=True)
    fill = []
    for rep in range(reps + 2):                      # the host copy of the maps into the pinned staging buffer
        t0 = time.perf_counter()
        flat = staging.numpy().view(np.uint16)
        for i, m in enumerate(maps):
            flat[i * H * W:(i + 1) * H * W] = m.reshape(-1)
        fill.append((time.perf_counter() - t0) * 1e3 / n)
    fill = fill[2:]
    ids = torch.empty(total, dtype=torch.int16, device=device)
    work = torch.empty(cs.workspace_bytes(n), dtype=torch.uint8, device=device)
    rows = torch.empty((n, cs.SLOTS, cs.COLUMNS), dtype=torch.int32, device=device)
    counts = torch.empty(n, dtype=torch.int32, device=device)
    rows_host = torch.empty(rows.shape, dtype=torch.int32, pin_memory=True)
    hw = np.ascontiguousarray([[H, W]] * n, dtype=np.int32)
    offsets = np.arange(n, dtype=np.int64) * (H * W)
    stream = torch.cuda.current_stream(device)
    up, run, down = [], [], []
    for rep in range(reps + 2):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        ids.copy_(staging, non_blocking=True)
        e[1].record()
        _lib.call("dadet_instance_boxes", ctypes.c_void_p(ids.data_ptr()), total, hw.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                  offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), n, ctypes.c_void_p(rows.data_ptr()),
                  ctypes.c_void_p(counts.data_ptr()), ctypes.c_void_p(work.data_ptr()), int(work.numel()),
                  ctypes.c_void_p(stream.cuda_stream))
        e[2].record()
        rows_host.copy_(rows, non_blocking=True)
        e[3].record()
        torch.cuda.synchronize()
        if rep >= 2:
            up.append(e[0].elapsed_time(e[1]) / n)
            run.append(e[1].elapsed_time(e[2]) / n)
            down.append(e[2].elapsed_time(e[3]) / n)
    print("batch of %2d maps, per map: staging fill (host) %.3f ms, upload %.3f ms, clear + accumulate + compact %.3f ms, "
          "rows back %.3f ms (medians of %d; %d instances in map 0)"
          % (n, median_ms(fill), median_ms(up), median_ms(run), median_ms(down), reps, int(counts[0])))


def host_times(maps, reps, tmp):
    from PIL import Image

    from da_detect_amd.data import cityscapes as cs

    path = os.path.join(tmp, "one_gtFine_instanceIds.png")
    Image.fromarray(maps[0]).save(path)
    table, decode = [], []
    for rep in range(reps + 2):
        t0 = time.perf_counter()
        cs.instance_table_host(maps[rep % len(maps)])
        t1 = time.perf_counter()
        cs.read_id_map(path)
        t2 = time.perf_counter()
        if rep >= 2:
            table.append((t1 - t0) * 1e3)
            decode.append((t2 - t1) * 1e3)
    print("host, per map: instance_table_host %.1f ms, Pillow decode of the 16-bit PNG (%d KiB) %.1f ms (medians of %d)"
          % (median_ms(table), os.path.getsize(path) // 1024, median_ms(decode), reps))


def split_times(maps, images, tmp):
    from PIL import Image

    from da_detect_amd.data import cityscapes as cs

    folder = os.path.join(tmp, "gtFine", "train", "city")
    os.makedirs(folder)
    for i in range(images):
        Image.fromarray(maps[i % len(maps)]).save(os.path.join(folder, "city_%06d_000019_gtFine_instanceIds.png" % i))
    results = {}
    for rounds in range(2):                          # each path twice, alternating: drift of the box shows as a difference
        for name, device in (("device", "cuda"), ("host", "cpu")):
            phases = {}
            t0 = time.perf_counter()
            results[name] = cs.build_annotations(os.path.join(tmp, "gtFine"), "train", device=device, timings=phases)
            wall = time.perf_counter() - t0
            print("split of %d maps, %s path: %.3f s wall = decode %.3f s + tables %.3f s + rest %.3f s (%d annotations), pass %d"
                  % (images, name, wall, phases["decode_s"], phases["tables_s"], wall - phases["decode_s"] - phases["tables_s"],
                     len(results[name]["annotations"]), rounds))
    assert results["device"] == results["host"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--reps", type=int, default=15)
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    maps = [synthetic_map(seed) for seed in range(16)]
    device_times(maps[:1], args.reps, device)
    device_times(maps, args.reps, device)
    with tempfile.TemporaryDirectory() as tmp:
        host_times(maps, args.reps, tmp)
        split_times(maps, args.images, tmp)


if __name__ == "__main__":
    main()
