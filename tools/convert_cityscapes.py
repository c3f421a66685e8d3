#!/usr/bin/env python
"""Cityscapes as unpacked from its archives -> the COCO-style box annotation files the catalog names refer to — the
counterpart of the reference's tools/cityscapes/convert_cityscapes_to_coco.py, convert_foggy_cityscapes_to_coco.py and
convert_cityscapes_to_caronly_coco.py, without cv2, cityscapesscripts, h5py or scipy (training does not need the files:
`cityscapes:ROOT,SPLIT` of tools/train_net_da.py reads the id maps itself):

    python tools/convert_cityscapes.py --datadir ROOT --outdir DIR \\
        --dataset cityscapes_instance_only|foggy_cityscapes|cityscapes_car_only [--beta B] [--splits train val] [--host] [--keep-fragmented]

ROOT holds gtFine/<split>/<city>/*_gtFine_instanceIds.png (and leftImg8bit[_foggy]/<split>/, looked at only to decide
whether `file_name` carries the city folder).  Per split one file with the reference's name is written to DIR:
instancesonly_filtered_gtFine_<split>.json, foggy_instancesonly_filtered_gtFine_<split>.json or
caronly_filtered_gtFine_<split>.json.  The boxes are computed on the HIP device when one is present (csrc/instance_boxes.hip),
with numpy otherwise or under --host; both write the same bytes.  Boxes only: there is no `segmentation` entry.
--keep-fragmented keeps the instances the reference drops as "invalid contours" (a component of at most 2 pixels)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DATASETS = {"cityscapes_instance_only": ("plain", False), "foggy_cityscapes": ("foggy", False),
            "cityscapes_car_only": ("plain", True)}


def main(argv=None):
    ap = argparse.ArgumentParser(description="COCO-style box annotations from raw Cityscapes")
    ap.add_argument("--datadir", required=True, help="the folder that holds gtFine/")
    ap.add_argument("--outdir", required=True)
    ap.add_argument("--dataset", choices=sorted(DATASETS), default="cityscapes_instance_only")
    ap.add_argument("--beta", type=float, default=0.02, help="foggy_cityscapes: 0.02 (default), 0.01 or 0.005")
    ap.add_argument("--splits", nargs="+", default=["train", "val"])
    ap.add_argument("--host", action="store_true", help="compute with numpy even when a HIP device is present")
    ap.add_argument("--keep-fragmented", action="store_true")
    args = ap.parse_args(argv)

    from da_detect_amd.data import cityscapes

    variant, car_only = DATASETS[args.dataset]
    on_device = cityscapes.device_available() and not args.host
    os.makedirs(args.outdir, exist_ok=True)
    for split in args.splits:
        data = cityscapes.build_annotations(
            os.path.join(args.datadir, "gtFine"), split, variant, args.beta, car_only, not args.keep_fragmented,
            os.path.join(args.datadir, cityscapes.IMAGE_DIRS[variant], split), "cuda" if on_device else "cpu")
        path = os.path.join(args.outdir, cityscapes.json_name(args.dataset, split))
        cityscapes.write_json(data, path)
        print("%s: %d images, %d annotations (%s)" % (path, len(data["images"]), len(data["annotations"]),
                                                      "device" if on_device else "host"))


if __name__ == "__main__":
    main()
