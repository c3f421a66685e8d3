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
`--expected TASK METRIC MEAN STD` (repeatable) is the reference's TEST.EXPECTED_RESULTS sanity band.

`--metric voc07` / `voc12` scores the same predictions PASCAL-VOC-style instead (AP per class and mAP at
`--voc-iou`, default 0.5; 11-point or area metric; a crowd annotation counts as `difficult`), which is the number the
domain-adaptation papers report, and writes `result.txt`.  `--dataset voc:DIR,SPLIT` names a set in PASCAL VOC layout; it has
no COCO form, so it is always scored VOC-style (`--metric coco` is then read as voc07, the reference's default), and with
`--config-file` its evaluation pass runs in this process (one GPU) and leaves `predictions.pth` in
`<output-dir>/inference/<DIR's name>_<SPLIT>/`: tools/test_net_da.py takes COCO-format sets only.
`--dataset cityscapes:ROOT,SPLIT[,foggy[=BETA]|rain][,caronly]` names Cityscapes as unpacked from its archives (data/cityscapes.py,
DESIGN.md 3h): a COCO-format set built from the id maps, scored with either metric.  With `--config-file` its annotations are
written to `<output-dir>/<ROOT's name>_<SPLIT and options>.json` first and that file, with the split's image folder, is what
tools/test_net_da.py (which takes annotation files) evaluates: `predictions.pth` lands in the folder of that name under
`<output-dir>/inference/`.

`--errors [--bg-iou 0.1]` adds, after the scoring, the error breakdown of the detections (every image's classes
matched at once on the device): per class and over all classes the detections by kind (TP, ignored, Cls, Loc, Both, Dupe,
Bkg), the missed ground truths, AP and the AP that fixing each kind alone would return, at `--voc-iou`'s first value, with
the 11-point metric unless `--metric voc12`; `errors.txt` and `errors.json` land next to the predictions.  It takes any of the
three kinds of set.  `--errors --compare OTHER/predictions.pth` logs a second table for that file and the difference per
kind: what adaptation fixed.

    python tools/score_net_da.py --dataset ann.json,imgdir --predictions noadapt/predictions.pth --metric voc07 --errors \\
        [--bg-iou 0.1] [--compare adapted/predictions.pth]

`--device-prep` (with `--config-file`): the evaluation pass runs in this process as well, for either kind of set, fed from the
device input pipeline — test-time augmentation through `TEST.BBOX_AUG.ENABLED True` included."""
import argparse
import logging
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from da_detect_amd.data.build import CITYSCAPES_PREFIX, dataset_from_spec, parse_dataset_spec  # noqa: E402
from da_detect_amd.data.evaluation import evaluate  # noqa: E402
from da_detect_amd.data.evaluation.voc import do_voc_evaluation  # noqa: E402


def _pair(text):
    if text.startswith(CITYSCAPES_PREFIX):       # cityscapes:ROOT,SPLIT[,foggy[=BETA]|rain][,caronly] (data/cityscapes.py)
        return parse_dataset_spec(text)
    ann, root = text.split(",")
    return ann, root


def _set_name(spec):
    """the folder under <output-dir>/inference a set's predictions go to"""
    for prefix in ("voc:", CITYSCAPES_PREFIX):
        if spec[0].startswith(prefix):
            return os.path.basename(spec[0][len(prefix):].rstrip("/")) + "_" + spec[1].replace(",", "_")
    return os.path.splitext(os.path.basename(spec[0]))[0]


def _evaluation_pass(args, folder):
    """the evaluation pass in this process — over a VOC-layout set (tools/test_net_da.py builds COCO records, which such a
    set has no ids for), or over any set with --device-prep (tools/test_net_da.py feeds from the host transforms only):
    detector, weights, test loader, engine.inference — it leaves predictions.pth in `folder`"""
    from da_detect_amd.config import cfg
    from da_detect_amd.data.build import make_test_data_loader
    from da_detect_amd.data.transforms import build_transforms
    from da_detect_amd.engine.inference import inference
    from da_detect_amd.modeling.detector import build_detection_model
    from da_detect_amd.utils.checkpoint import DetectronCheckpointer

    if not torch.cuda.is_available():
        raise SystemExit("score_net_da.py needs a HIP device: the product path has no CPU fallback")
    c = cfg.clone()
    c.merge_from_file(args.config_file)
    c.merge_from_list(args.opts)
    c.freeze()
    device = torch.device("cuda", torch.cuda.current_device())
    model = build_detection_model(c).to(device)
    DetectronCheckpointer(c, model, save_dir=args.output_dir).load(args.ckpt if args.ckpt else c.MODEL.WEIGHT)
    model.eval()
    dataset = dataset_from_spec(args.dataset, build_transforms(c, is_train=False), is_train=False)
    os.makedirs(folder, exist_ok=True)
    inference(model, make_test_data_loader(c, dataset, device_prep=args.device_prep), dataset_name=",".join(args.dataset),
              box_only=c.MODEL.RPN_ONLY, device=device, output_folder=folder,
              evaluate=lambda **_: None)      # scored below, from the saved file


def build_parser():
    ap = argparse.ArgumentParser(description="COCO box AP / proposal recall of saved predictions, on MI355X")
    ap.add_argument("--dataset", type=_pair, required=True,
                    help="annotation.json,image_root of the test set — or voc:DIR,SPLIT, or "
                         "cityscapes:ROOT,SPLIT[,foggy[=BETA]|rain][,caronly]")
    ap.add_argument("--predictions", default=None, help="predictions.pth written by tools/test_net_da.py")
    ap.add_argument("--config-file", default=None, help="run tools/test_net_da.py with this yaml first, then score its output")
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--output-dir", default=None)
    ap.add_argument("--proposals", action="store_true", help="score proposal recall instead of box AP")
    ap.add_argument("--expected", nargs=4, action="append", default=[], metavar=("TASK", "METRIC", "MEAN", "STD"))
    ap.add_argument("--sigma-tol", type=float, default=4)
    ap.add_argument("--metric", choices=("coco", "voc07", "voc12"), default="coco",
                    help="coco: COCO box AP (default); voc07 / voc12: PASCAL VOC AP, 11-point / area metric")
    ap.add_argument("--voc-iou", type=float, nargs="+", default=[0.5], help="IoU threshold(s) of the VOC metrics")
    ap.add_argument("--device-prep", action="store_true",
                    help="with --config-file: the evaluation pass runs in this process (one GPU) and prepares its batches — and, "
                         "with TEST.BBOX_AUG.ENABLED True, every augmentation pass — on the device from decoded uint8 pixels "
                         "(data/device_prep.py); same inputs as the host transforms, bit for bit")
    ap.add_argument("--errors", action="store_true",
                    help="after the scoring: the error breakdown of the detections (kinds, missed, dAP per fix) at --voc-iou's "
                         "first value, 11-point metric unless --metric voc12; writes errors.txt and errors.json")
    ap.add_argument("--bg-iou", type=float, default=0.1, help="with --errors: below this IoU a detection touches nothing")
    ap.add_argument("--compare", default=None, metavar="PREDICTIONS",
                    help="with --errors: a second predictions.pth of the same set; its table and the differences are logged")
    ap.add_argument("opts", nargs=argparse.REMAINDER, help="KEY VALUE overrides of the yaml (with --config-file)")
    return ap


def _error_tables(args, dataset, predictions, folder, log):
    """--errors: the breakdown of `predictions` (written next to them), then that of --compare and what changed"""
    from da_detect_amd.data.evaluation import errors

    settings = dict(pos_thresh=args.voc_iou[0], bg_thresh=args.bg_iou, use_07_metric=args.metric != "voc12")
    first = errors.do_error_analysis(dataset, predictions, folder, log, **settings)
    if args.compare is None:
        return
    other = torch.load(args.compare, weights_only=False)
    if len(other) != len(dataset):
        raise SystemExit("%s: %d predictions for %d images: not this dataset's predictions.pth" % (args.compare, len(other), len(dataset)))
    log.info("--compare %s", args.compare)
    second = errors.do_error_analysis(dataset, other, None, log, **settings)
    rows = ["{:<8}{:>12}{:>12}{:>12}".format("", "predictions", "compare", "difference")]
    for k, name in enumerate(errors.KIND_NAMES):
        a, b = int(first["counts"][1:, k].sum()), int(second["counts"][1:, k].sum())
        rows.append("{:<8}{:>12d}{:>12d}{:>+12d}".format(name, a, b, b - a))
    a, b = int(first["missed"][1:].sum()), int(second["missed"][1:].sum())
    rows.append("{:<8}{:>12d}{:>12d}{:>+12d}".format("missed", a, b, b - a))
    rows.append("{:<8}{:>12.4f}{:>12.4f}{:>+12.4f}".format("mAP", first["map"], second["map"], second["map"] - first["map"]))
    for name in errors.FIXES:
        a, b = first["dap"][name], second["dap"][name]
        rows.append("{:<8}{:>+12.4f}{:>+12.4f}{:>+12.4f}".format("d" + name, a, b, b - a))
    log.info("what changed (compare - predictions)\n%s", "\n".join(rows))


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.compare is not None and not args.errors:
        raise SystemExit("--compare goes with --errors")
    if args.errors and args.proposals:
        raise SystemExit("--errors breaks down detections, not proposals")
    if (args.predictions is None) == (args.config_file is None):
        raise SystemExit("give either --predictions (score a saved file) or --config-file with --output-dir (evaluate, then score)")
    if args.config_file is not None:
        if not args.output_dir:
            raise SystemExit("--config-file needs --output-dir: the evaluation pass leaves predictions.pth there")
        logging.basicConfig(level=logging.INFO)
        if args.dataset[0].startswith(CITYSCAPES_PREFIX):
            # a COCO-format set: its annotations are written out once, as <output-dir>/<set name>.json, and from here on it is an
            # (annotation file, image root) pair like any other — tools/test_net_da.py evaluates it, in its own process
            from da_detect_amd.data.cityscapes import write_annotation_file

            os.makedirs(args.output_dir, exist_ok=True)
            args.dataset = write_annotation_file(args.dataset[0][len(CITYSCAPES_PREFIX):], args.dataset[1],
                                                 os.path.join(args.output_dir, _set_name(args.dataset) + ".json"))
        folder = os.path.join(args.output_dir, "inference", _set_name(args.dataset))
        if args.dataset[0].startswith("voc:") or args.device_prep:
            _evaluation_pass(args, folder)
        else:
            run = [sys.executable, os.path.join(ROOT, "tools", "test_net_da.py"), "--config-file", args.config_file, "--dataset",
                   ",".join(args.dataset), "--output-dir", args.output_dir] + (["--ckpt", args.ckpt] if args.ckpt else []) + args.opts
            subprocess.check_call(run)
        args.predictions = os.path.join(folder, "predictions.pth")
        rpn_only = [v for k, v in zip(args.opts[::2], args.opts[1::2]) if k == "MODEL.RPN_ONLY"]
        args.proposals = args.proposals or (bool(rpn_only) and rpn_only[-1].lower() in ("true", "1"))
    if not args.proposals and not torch.cuda.is_available():
        raise SystemExit("score_net_da.py needs a HIP device: box AP is matched on it, there is no CPU fallback")

    logging.basicConfig(level=logging.INFO)
    log = logging.getLogger("maskrcnn_benchmark.score_net")
    ann, root = args.dataset
    dataset = dataset_from_spec(args.dataset, None, is_train=False)
    predictions = torch.load(args.predictions, weights_only=False)
    if len(predictions) != len(dataset):
        raise SystemExit("%d predictions for %d images: not this dataset's predictions.pth" % (len(predictions), len(dataset)))
    folder = os.path.dirname(os.path.abspath(args.predictions))
    if not args.proposals and (args.metric != "coco" or ann.startswith("voc:")):
        result = do_voc_evaluation(dataset, predictions, folder, log, iou_thresh=args.voc_iou[0] if len(args.voc_iou) == 1
                                   else args.voc_iou, use_07_metric=args.metric != "voc12")
        for iou, row in zip(args.voc_iou, result.get("ap_by_iou", ())):
            log.info("IoU %.2f: mAP %.4f", iou, float(row[row == row].mean()) if (row == row).any() else float("nan"))
        if args.errors:
            _error_tables(args, dataset, predictions, folder, log)
        return
    expected = [(task, metric, (float(mean), float(std))) for task, metric, mean, std in args.expected]
    out = evaluate(dataset, predictions, folder, box_only=args.proposals,
                   iou_types=("bbox",), expected_results=expected, expected_results_sigma_tol=args.sigma_tol)
    if out is not None:
        results, records = out
        log.info("%d detections on %d images", len(records["bbox"]), len(dataset))
        log.info("COCO box AP (rows: all categories, then each json category id)\n%s", results.table())
    if args.errors and not args.proposals:
        _error_tables(args, dataset, predictions, folder, log)


if __name__ == "__main__":
    main()
