#!/usr/bin/env python
"""ms per step, images/s and peak memory of the `da` and `triplet` recipes with k images per domain on one GPU.

    python tools/probes/images_per_gpu.py [--workloads da,triplet] [--steps 20] [--warmup 10] [--image-hw 1024x2048]

Each (recipe, k) runs in a child process of its own (a fresh allocator and fresh caches: torch.cuda.max_memory_allocated is
then that configuration's own peak), built and timed exactly as bench.py times its step: bench.build with seed 100, the
overlapped RPN backward, the wgrad-lane tuner's untimed steps, `--warmup` steps, then `--steps` steps of train_step between
two synchronisations.  The batch is make_batch(..., 2k or 3k images, num_source = k): [S_1..S_k, T_1..T_k(, A_1..A_k)].
k = 1 is bench.py's own batch: that row must agree with `python bench.py --workload da` / `triplet` of the same commit
within the run-to-run spread — the probe's sanity check.  da: k = 1, 2, 4; triplet: k = 1, 2 (the range in which the image
head's loss sums take the fixed-order path, 8 images)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
KS = {"da": (1, 2, 4), "triplet": (1, 2)}


def one(name, k, steps, warmup, hw):
    import bench  # (sets HIP_FORCE_DEV_KERNARG before the runtime starts, as the benchmark does)
    import torch

    from da_detect_amd.data.synthetic import make_batch
    from da_detect_amd.engine.trainer import WgradLaneTuner, enable_overlapped_rpn_backward, train_step
    from da_detect_amd.utils import streams

    device = torch.device("cuda:0")
    yaml_path, overrides, per_gpu, _ = bench.WORKLOADS[name]
    height, width = hw
    c, model, opt, _ = bench.build(yaml_path, device, seed=100, overrides=overrides)
    enable_overlapped_rpn_backward(model, True)
    images, targets = make_batch(c, per_gpu * k, height, width, seed=100, device=device, num_source=k)
    streams.join_wgrad_lane(device)
    streams.WGRAD_LANE_ROWS = int(os.environ.get("DADET_WGRAD_LANE_ROWS", "0"))
    tuner = WgradLaneTuner(device)
    while tuner.active:
        tuner.step_begin()
        train_step(model, opt, images, targets)
        tuner.step_end()
    for _ in range(warmup):
        train_step(model, opt, images, targets)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        losses = train_step(model, opt, images, targets)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    finite = all(bool(torch.isfinite(v.detach()).all()) for v in losses.values())
    print(json.dumps({"workload": name, "k": k, "images": per_gpu * k, "ms_per_step": round(ms, 3),
                      "images_per_s": round(per_gpu * k / ms * 1e3, 2),
                      "max_memory_allocated_GB": round(torch.cuda.max_memory_allocated(device) / 2 ** 30, 2),
                      "losses_finite": finite, "steps": steps, "warmup": warmup, "image_hw": "%dx%d" % (height, width)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="da,triplet")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--image-hw", default="1024x2048")
    ap.add_argument("--ks", default=None, help="comma-separated k values (default: da 1,2,4; triplet 1,2)")
    ap.add_argument("--child", nargs=2, metavar=("WORKLOAD", "K"), default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    hw = tuple(int(v) for v in args.image_hw.lower().split("x"))
    if args.child:
        one(args.child[0], int(args.child[1]), args.steps, args.warmup, hw)
        return
    rows = []
    for name in args.workloads.split(","):
        for k in ([int(v) for v in args.ks.split(",")] if args.ks else KS[name]):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", name, str(k), "--steps", str(args.steps),
                   "--warmup", str(args.warmup), "--image-hw", args.image_hw]
            out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
            line = [l for l in out.stdout.splitlines() if l.startswith("{")]
            if out.returncode != 0 or not line:
                print("%s k=%d failed (exit %d):\n%s" % (name, k, out.returncode, out.stderr[-2000:]))
                sys.exit(out.returncode or 1)       # nothing further is started on the GPU after a failure
            rows.append(json.loads(line[-1]))
            print(line[-1], flush=True)
    print("%-8s %2s %6s %12s %10s %12s" % ("recipe", "k", "images", "ms per step", "images/s", "peak GB"))
    for r in rows:
        print("%-8s %2d %6d %12.2f %10.2f %12.2f" % (r["workload"], r["k"], r["images"], r["ms_per_step"],
                                                    r["images_per_s"], r["max_memory_allocated_GB"]))


if __name__ == "__main__":
    main()
