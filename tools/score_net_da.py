#!/usr/bin/env python
"""Evaluate and score in one command, or score what tools/test_net_da.py wrote: COCO box AP for all categories and per
category, or proposal recall.

tools/test_net_da.py runs the detector over a test set and leaves `predictions.pth` (one BoxList per image) and
`bbox.json` in `<output-dir>/inference/<annotation name>/`; it is kept as it is.  This tool scores that `predictions.pth`
with this package's own scorer (da_detect_amd/data/evaluation: the matching of COCO's bbox evaluation in one launch on the
device, DESIGN.md 3d — no pycocotools), logs the table and writes `coco_results.pth` (and `bbox.json` again, identical)
next to it.  With `--config-file` it first runs tools/test_net_da.py itself, in a process of its own, with the same
dataset, `--ckpt`, `--output-dir` and KEY VALUE overrides, so the per-class table comes out of one command:

    python tools/score_net_da.py --dataset ann.json,imgdir --config-file configs/da_faster_rcnn/<yaml> --output-dir out \\
        [--ckpt model_final.pth] [KEY VALUE ...]
    python tools/score_net_da.py --dataset ann.json,imgdir --predictions out/inference/<name>/predictions.pth [--proposals]

`--proposals`: the predictions are RPN proposals with an `objectness` field; AR at 100 and 1000 proposals for four area
ranges is logged and `box_proposals.pth` written.  With `--config-file` it is implied by `MODEL.RPN_ONLY True` among the
overrides (the evaluation pass itself then already logs the recalls: engine/inference.py sends proposals there).
`--expected TASK METRIC MEAN STD` (repeatable) is the reference's TEST.EXPECTED_RESULTS sanity band."""
import argparse
import logging
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from da_detect_amd.data.datasets import COCODataset  # noqa: E402
from da_detect_amd.data.evaluation import evaluate  # noqa: E402


def _pair(text):
    ann, root = text.split(",")
    return ann, root


def main():
    ap = argparse.ArgumentParser(description="COCO box AP / proposal recall of saved predictions, on MI355X")
    ap.add_argument("--dataset", type=_pair, required=True, help="annotation.json,image_root of the test set")
    ap.add_argument("--predictions", default=None, help="predictions.pth written by tools/test_net_da.py")
    ap.add_argument("--config-file", default=None, help="run tools/test_net_da.py with this yaml first, then score its output")
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--output-dir", default=None)
    ap.add_argument("--proposals", action="store_true", help="score proposal recall instead of box AP")
    ap.add_argument("--expected", nargs=4, action="append", default=[], metavar=("TASK", "METRIC", "MEAN", "STD"))
    ap.add_argument("--sigma-tol", type=float, default=4)
    ap.add_argument("opts", nargs=argparse.REMAINDER, help="KEY VALUE overrides of the yaml (with --config-file)")
    args = ap.parse_args()
    if (args.predictions is None) == (args.config_file is None):
        raise SystemExit("give either --predictions (score a saved file) or --config-file with --output-dir (evaluate, then score)")
    if args.config_file is not None:
        if not args.output_dir:
            raise SystemExit("--config-file needs --output-dir: the evaluation pass leaves predictions.pth there")
        run = [sys.executable, os.path.join(ROOT, "tools", "test_net_da.py"), "--config-file", args.config_file, "--dataset",
               ",".join(args.dataset), "--output-dir", args.output_dir] + (["--ckpt", args.ckpt] if args.ckpt else []) + args.opts
        subprocess.check_call(run)
        name = os.path.splitext(os.path.basename(args.dataset[0]))[0]
        args.predictions = os.path.join(args.output_dir, "inference", name, "predictions.pth")
        rpn_only = [v for k, v in zip(args.opts[::2], args.opts[1::2]) if k == "MODEL.RPN_ONLY"]
        args.proposals = args.proposals or (bool(rpn_only) and rpn_only[-1].lower() in ("true", "1"))
    if not args.proposals and not torch.cuda.is_available():
        raise SystemExit("score_net_da.py needs a HIP device: box AP is matched on it, there is no CPU fallback")

    logging.basicConfig(level=logging.INFO)
    log = logging.getLogger("maskrcnn_benchmark.score_net")
    ann, root = args.dataset
    dataset = COCODataset(ann, root, remove_images_without_annotations=False)
    predictions = torch.load(args.predictions, weights_only=False)
    if len(predictions) != len(dataset):
        raise SystemExit("%d predictions for %d images: not this dataset's predictions.pth" % (len(predictions), len(dataset)))
    expected = [(task, metric, (float(mean), float(std))) for task, metric, mean, std in args.expected]
    out = evaluate(dataset, predictions, os.path.dirname(os.path.abspath(args.predictions)), box_only=args.proposals,
                   iou_types=("bbox",), expected_results=expected, expected_results_sigma_tol=args.sigma_tol)
    if out is not None:
        results, records = out
        log.info("%d detections on %d images", len(records["bbox"]), len(dataset))
        log.info("COCO box AP (rows: all categories, then each json category id)\n%s", results.table())


if __name__ == "__main__":
    main()
