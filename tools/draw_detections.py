#!/usr/bin/env python
"""Draw ground truth and detections onto a test set's images: one PNG per image, its panels stacked top to bottom.

    python tools/draw_detections.py --dataset ann.json,imgdir --predictions out/inference/<name>/predictions.pth --out figs \\
        [--gt] [--compare other/predictions.pth ...] [--threshold 0.7] [--limit N] [--ids ID ...]
        [--thickness 2] [--fill-alpha 0] [--no-scores] [--host] [--errors [--errors-iou 0.5] [--bg-iou 0.1]]
    python tools/draw_detections.py --dataset ann.json,imgdir --config-file configs/da_faster_rcnn/<yaml> --ckpt model_final.pth \\
        --out figs [KEY VALUE ...]

Panels, in this order: the ground truth (`--gt`), the predictions, then every `--compare` set — each the original image with
its own overlay, so `--gt --predictions noadapt.pth --compare adapted.pth` is the "ground truth / no adaptation / adapted"
figure of a domain-adaptation paper in one call.  `--dataset` is `ann.json,imgdir`, `voc:DIR,SPLIT` or
`cityscapes:ROOT,SPLIT[,foggy[=BETA]|rain][,caronly]`, as for the other tools; class names are the dataset's.  A prediction
file is what tools/test_net_da.py / tools/score_net_da.py leave behind (one BoxList per image); its boxes are resized to the
original image exactly as the scorers do (engine/inference.py prepare_for_coco_detection), and the ones with a score above
`--threshold` are drawn, the most confident on top.  With `--config-file` the evaluation pass runs first, in this process on
one GPU (tools/score_net_da.py's), and leaves `predictions.pth` in `<out>/inference/<set name>/`.

`--errors` colours every predictions panel by the KIND of each detection's error instead of by class (one fixed
table of seven colours in data/evaluation/errors.py: TP, ignored, Cls, Loc, Both, Dupe, Bkg), labels a box
"<class> <score> <Kind>", and adds the image's missed ground truths in an eighth colour, labelled "missed <class>".  The kinds
come from ALL detections of the selected images, matched on the device in one launch per prediction file (so this needs a HIP
device, with or without `--host`); `--threshold` only decides which of them are drawn.

The drawing rules are engine/overlay.py's.  The panels are drawn on the device (csrc/overlay.hip, all panels
of an image in one launch) when there is one and `--host` is not given, otherwise by the numpy renderer: the files are the
same either way.  `--ids` selects images by their dataset id (the json's image id, the VOC split's image name), `--limit`
keeps the first N of the selection.  A file is named after the image: `<out>/<image file's stem>.png`."""
import argparse
import logging
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from da_detect_amd.data.build import dataset_from_spec  # noqa: E402
from da_detect_amd.engine import overlay  # noqa: E402
from score_net_da import _evaluation_pass, _pair, _set_name  # noqa: E402


class DatasetNames(object):
    """label -> class name of a dataset, in the form build_draw_list takes"""

    def __init__(self, dataset):
        self.dataset = dataset

    def __getitem__(self, label):
        return self.dataset.map_class_id_to_class_name(label).strip()


def image_stem(dataset, index):
    info = dataset.get_img_info(index)
    if "file_name" in info:
        return os.path.splitext(os.path.basename(info["file_name"]))[0]
    return str(dataset.id_to_img_map[index])


def select_images(dataset, ids, limit):
    chosen = list(range(len(dataset)))
    if ids:
        wanted = set(str(i) for i in ids)
        chosen = [i for i in chosen if str(dataset.id_to_img_map[i]) in wanted]
        missing = wanted - set(str(dataset.id_to_img_map[i]) for i in chosen)
        if missing:
            raise SystemExit("--ids: not in the dataset: %s" % ", ".join(sorted(missing)))
    return chosen[:limit] if limit is not None else chosen


def error_kinds(dataset, chosen, predictions, args):
    """--errors: image index -> (kind of every detection in record order, state of every ground truth), from ALL detections
    of the chosen images in one launch (data/evaluation/errors.py); the score threshold only decides what is drawn"""
    from da_detect_amd.data.evaluation import errors

    sizes = [dataset.get_img_info(i) for i in chosen]
    packed = errors.pack([predictions[i].resize((s["width"], s["height"])) for i, s in zip(chosen, sizes)],
                         [dataset.get_groundtruth(i) for i in chosen])
    return dict(zip(chosen, errors.per_image(packed, errors.match(packed, args.errors_iou, args.bg_iou))))


def error_panel(dataset, index, prediction, kinds, names, args, style):
    """one predictions panel of --errors: the image's missed ground truths (underneath), then the detections above the score
    threshold, coloured by kind and labelled "<class> <score> <Kind>" """
    from da_detect_amd.data.evaluation import errors

    kind, state = kinds
    truth = dataset.get_groundtruth(index)
    missed = truth[torch.from_numpy(np.flatnonzero(state == errors.MISSED))].copy_with_fields(["labels"])
    texts = ["missed %s" % names[int(k)] for k in missed.get_field("labels").tolist()]
    missed.add_field("labels", torch.arange(len(missed)))
    records = overlay.build_draw_list(missed, texts, colors=np.tile(np.asarray(errors.MISSED_COLOR, dtype=np.uint8), (len(missed), 1)),
                                      **style)
    prediction.add_field("kinds", torch.from_numpy(kind.astype(np.int64)))
    top = overlay.select_top_predictions(prediction, args.threshold)
    top_kind = top.get_field("kinds").tolist()
    texts = [names[int(k)] if args.no_scores else "%s %.2f" % (names[int(k)], s)
             for k, s in zip(top.get_field("labels").tolist(), top.get_field("scores").tolist())]
    texts = ["%s %s" % (t, errors.KIND_NAMES[k]) for t, k in zip(texts, top_kind)]
    top.add_field("labels", torch.arange(len(top)))
    colors = np.asarray(errors.KIND_COLORS, dtype=np.uint8)[np.asarray(top_kind, dtype=np.int64)].reshape(-1, 3)
    return records + overlay.build_draw_list(top, texts, show_scores=False, colors=colors, **style)


def panel_lists(dataset, index, target, size, prediction_sets, args, kinds=None):
    """the draw list of every panel of image `index`, top to bottom; kinds: per prediction set, error_kinds' answer"""
    names = DatasetNames(dataset)
    style = dict(thickness=args.thickness, fill_alpha=args.fill_alpha)
    lists = []
    if args.gt:
        lists.append(overlay.build_draw_list(target.copy_with_fields(["labels"]), names, **style))
    for which, predictions in enumerate(prediction_sets):
        if kinds is not None:
            lists.append(error_panel(dataset, index, predictions[index].resize(size), kinds[which][index], names, args, style))
            continue
        top = overlay.select_top_predictions(predictions[index].resize(size), args.threshold)
        lists.append(overlay.build_draw_list(top, names, show_scores=not args.no_scores, **style))
    return lists


def draw_panels(pixels, lists, device):
    """uint8 [H, W, 3] array + draw lists -> the panels stacked top to bottom"""
    if device is None:
        return np.concatenate([overlay.render_host(pixels, records) for records in lists], axis=0)
    stack = torch.from_numpy(pixels).to(device).unsqueeze(0).repeat(len(lists), 1, 1, 1)
    overlay.render_device(list(stack.unbind(0)), lists)
    return stack.reshape(-1, pixels.shape[1], 3).cpu().numpy()


def build_parser():
    ap = argparse.ArgumentParser(description="ground truth and detections drawn onto a test set's images, one PNG per image")
    ap.add_argument("--dataset", type=_pair, required=True,
                    help="annotation.json,image_root of the test set — or voc:DIR,SPLIT, or "
                         "cityscapes:ROOT,SPLIT[,foggy[=BETA]|rain][,caronly]")
    ap.add_argument("--predictions", default=None, help="predictions.pth written by tools/test_net_da.py")
    ap.add_argument("--config-file", default=None, help="run the evaluation pass with this yaml first, then draw its output")
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--out", required=True, help="folder the PNG files go to")
    ap.add_argument("--threshold", type=float, default=0.7, help="draw the detections with a score above this")
    ap.add_argument("--gt", action="store_true", help="first panel: the ground truth")
    ap.add_argument("--compare", nargs="+", default=[], metavar="PREDICTIONS", help="further prediction files, a panel each")
    ap.add_argument("--limit", type=int, default=None, help="the first N images of the selection")
    ap.add_argument("--ids", nargs="+", default=[], help="dataset ids of the images to draw")
    ap.add_argument("--thickness", type=int, default=2)
    ap.add_argument("--fill-alpha", type=int, default=0, help="box tint, 0 (none) .. 256 (solid)")
    ap.add_argument("--no-scores", action="store_true", help="label = the class name alone")
    ap.add_argument("--host", action="store_true", help="draw with the numpy renderer even where there is a HIP device")
    ap.add_argument("--errors", action="store_true",
                    help="colour the detections by the kind of their error, not by class, and add the missed ground truths")
    ap.add_argument("--errors-iou", type=float, default=0.5, help="with --errors: the IoU a correct detection reaches")
    ap.add_argument("--bg-iou", type=float, default=0.1, help="with --errors: below this IoU a detection touches nothing")
    ap.add_argument("opts", nargs=argparse.REMAINDER, help="KEY VALUE overrides of the yaml (with --config-file)")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    if (args.predictions is None) == (args.config_file is None):
        raise SystemExit("give either --predictions (draw a saved file) or --config-file (evaluate, then draw)")
    logging.basicConfig(level=logging.INFO)
    log = logging.getLogger("maskrcnn_benchmark.draw_detections")
    if args.config_file is not None:
        if not torch.cuda.is_available():
            raise SystemExit("draw_detections.py --config-file needs a HIP device: the evaluation pass has no CPU fallback")
        args.output_dir, args.device_prep = args.out, True
        folder = os.path.join(args.out, "inference", _set_name(args.dataset))
        _evaluation_pass(args, folder)
        args.predictions = os.path.join(folder, "predictions.pth")

    dataset = dataset_from_spec(args.dataset, None, is_train=False)
    prediction_sets = []
    for path in [args.predictions] + list(args.compare):
        predictions = torch.load(path, weights_only=False)
        if len(predictions) != len(dataset):
            raise SystemExit("%s: %d predictions for %d images: not this dataset's predictions.pth"
                             % (path, len(predictions), len(dataset)))
        prediction_sets.append(predictions)
    device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() and not args.host else None
    os.makedirs(args.out, exist_ok=True)
    from PIL import Image

    written = []
    chosen = select_images(dataset, args.ids, args.limit)
    kinds = None
    if args.errors:
        if not torch.cuda.is_available():
            raise SystemExit("draw_detections.py --errors needs a HIP device: the kinds are matched on it (--host only draws)")
        kinds = [error_kinds(dataset, chosen, predictions, args) for predictions in prediction_sets]
    for index in chosen:
        img, target, _ = dataset[index]
        pixels = np.array(img, dtype=np.uint8)
        info = dataset.get_img_info(index)
        lists = panel_lists(dataset, index, target, (info["width"], info["height"]), prediction_sets, args, kinds)
        path = os.path.join(args.out, image_stem(dataset, index) + ".png")
        Image.fromarray(draw_panels(pixels, lists, device)).save(path)
        written.append(path)
    log.info("%d images drawn to %s (%s renderer)", len(written), args.out, "host" if device is None else "device")
    return written


if __name__ == "__main__":
    main()
