#!/usr/bin/env python
"""Write the rainy rendering of a dataset's images to disk — the offline counterpart of the reference's
efficientderain-master/generate_rainy_cityscape.py, without OpenCV (training does not need it: `--auxiliary rain:MASKDIR`
of tools/train_net_da.py synthesises the rain per sample):

    python tools/synthesize_rain.py --dataset ann.json,imgdir --masks DIR --out DIR [--seed N] [--host]

Every image of the dataset (`voc:DIR,SPLIT` for PASCAL VOC layout) is blended with one rain mask of --masks under one
drawn plan (da_detect_amd/data/rain.py) and saved as PNG under --out, at its file's relative path with the extension
replaced.  The rain is synthesised on the HIP device when one is present, with Pillow and numpy otherwise or under --host;
both give the same bytes.  --seed (default 0) seeds Python's `random`, from which every image draws its mask and the seed
of its plan: one seed, one rainy set."""
import argparse
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def _pair(text):
    first, second = text.split(",")
    return first, second


def relative_name(dataset, index):
    """where the image of sample `index` lives below the dataset's image root"""
    if hasattr(dataset, "imgs"):
        return dataset.imgs[dataset.id_to_img_map[index]]["file_name"]
    return dataset.ids[index] + ".jpg"


def main(argv=None):
    ap = argparse.ArgumentParser(description="synthesise the rainy rendering of a dataset")
    ap.add_argument("--dataset", type=_pair, required=True, help="ann.json,imgdir — or voc:DIR,SPLIT")
    ap.add_argument("--masks", required=True, help="folder of rain-mask images")
    ap.add_argument("--out", required=True, help="folder the rainy PNG files are written to")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--host", action="store_true", help="synthesise with Pillow and numpy even when a HIP device is present")
    args = ap.parse_args(argv)

    import torch
    from PIL import Image

    from da_detect_amd.data import rain
    from da_detect_amd.data.build import dataset_from_spec

    dataset = dataset_from_spec(args.dataset, None, is_train=False)
    masks = rain.RainMasks(args.masks)
    on_device = torch.cuda.is_available() and not args.host
    device = torch.device("cuda", torch.cuda.current_device()) if on_device else None
    random.seed(args.seed)
    for index in range(len(dataset)):
        img = dataset[index][0]                      # (no transforms: the PIL image)
        mask_index = random.randrange(len(masks))
        plan = rain.draw_rain_plan(np.random.RandomState(random.getrandbits(32)), img.size[0], img.size[1])
        pixels = np.array(img, dtype=np.uint8)
        if on_device:
            rainy = rain.synthesize_device(rain.upload(pixels, device), masks.device_mask(mask_index, img.size, device),
                                           plan).cpu().numpy()
        else:
            rainy = rain.synthesize_host(pixels, masks.host_mask(mask_index, img.size), plan)
        path = os.path.join(args.out, os.path.splitext(relative_name(dataset, index))[0] + ".png")
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        Image.fromarray(rainy).save(path)
    print("%d rainy images written to %s (%s)" % (len(dataset), args.out, "device" if on_device else "host"))


if __name__ == "__main__":
    main()
