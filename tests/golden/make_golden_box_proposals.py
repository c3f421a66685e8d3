"""Golden record for proposal recall — runs ONLY in the authoring container (needs /root/reference).

Calls the reference's own `evaluate_box_proposals` (maskrcnn_benchmark/data/datasets/evaluation/coco/coco_eval.py) on six
small seeded images and stores inputs and outputs in tests/golden/box_proposals.json: image sizes, annotations (areas in the
small, medium and large ranges and in the four upper sub-ranges, two crowd boxes, one image without ground truth), proposals
with an `objectness` field (one image without proposals, one with 150 so that the limit of 100 bites, sizes that differ from
the image's so the resize is exercised), and for every area range and both limits what the function returned.

What is substituted, all of it here and none of it in ref_shims.py or the reference:
  * the reference reads its ground truth through a pycocotools `COCO` object; the stand-in below answers the two calls the
    function makes (`getAnnIds(imgIds=)`, `loadAnns`) from the same annotation list;
  * the reference's package __init__ files on the way to coco_eval.py pull in torchvision and its datasets; the packages
    are registered as bare namespaces over the reference's directories, so only coco_eval.py, structures/bounding_box.py
    and structures/boxlist_ops.py are executed.  `Masker` (imported by coco_eval.py for masks, never called here) and tqdm
    (when not installed) are empty stand-ins, `maskrcnn_benchmark.layers.nms` is the reference's compiled CPU NMS.

    python tests/golden/make_golden_box_proposals.py
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import ref_shims  # noqa: E402


class _Coco(object):
    def __init__(self, annotations):
        self.anns = {a["id"]: a for a in annotations}

    def getAnnIds(self, imgIds):
        return [a["id"] for a in self.anns.values() if a["image_id"] == imgIds]

    def loadAnns(self, ids):
        return [self.anns[i] for i in ids]


class _Dataset(object):
    def __init__(self, images, annotations):
        self.images = images
        self.coco = _Coco(annotations)
        self.id_to_img_map = {i: im["id"] for i, im in enumerate(images)}

    def get_img_info(self, index):
        return self.images[index]


def _bare_packages(ref_c):
    """maskrcnn_benchmark's packages as bare namespaces over the reference tree (see the module docstring)"""
    base = os.path.join(ref_shims.REF_ROOT, "maskrcnn_benchmark")
    for name in [n for n in sys.modules if n == "maskrcnn_benchmark" or n.startswith("maskrcnn_benchmark.")]:
        del sys.modules[name]
    for sub in ("", ".structures", ".data", ".data.datasets", ".data.datasets.evaluation", ".data.datasets.evaluation.coco",
                ".modeling", ".modeling.roi_heads", ".modeling.roi_heads.mask_head"):
        m = types.ModuleType("maskrcnn_benchmark" + sub)
        m.__path__ = [os.path.join(base, *[p for p in sub.split(".") if p])]
        sys.modules[m.__name__] = m
    layers = types.ModuleType("maskrcnn_benchmark.layers")
    layers.nms = ref_c.nms
    masks = types.ModuleType("maskrcnn_benchmark.modeling.roi_heads.mask_head.inference")
    masks.Masker = type("Masker", (object,), {})
    sys.modules.update({"maskrcnn_benchmark.layers": layers, "maskrcnn_benchmark._C": ref_c, masks.__name__: masks})
    try:
        import tqdm  # noqa: F401
    except ImportError:
        stand_in = types.ModuleType("tqdm")
        stand_in.tqdm = lambda it, *a, **k: it
        sys.modules["tqdm"] = stand_in


def make_inputs(seed=11):
    rng = np.random.default_rng(seed)
    images = [{"id": 40 + i, "file_name": "p%d.png" % i, "width": 1400, "height": 1100} for i in range(6)]
    sides = [12, 25, 40, 80, 100, 120, 180, 300, 560, 700]     # areas across all eight ranges
    annotations, proposals = [], []
    for i, im in enumerate(images):
        gts = []
        if i != 2:                                             # image 2: no ground truth
            for j in range(4 + 2 * i):
                side = sides[(3 * i + j) % len(sides)]
                w, h = side, int(side * [1.0, .8, 1.25][j % 3])
                x, y = int(rng.integers(0, 1400 - w)), int(rng.integers(0, 1100 - h))
                gts.append([x, y, w, h])
                annotations.append({"id": len(annotations) + 1, "image_id": im["id"], "category_id": 1 + j % 2,
                                    "bbox": [x, y, w, h], "area": float(w * h) * [1.0, .7][j % 2],
                                    "iscrowd": 1 if (i, j) in ((0, 1), (4, 3)) else 0})
        size = (700, 550) if i % 2 else (1400, 1100)           # proposals live in the network-input size
        scale = size[0] / 1400.0
        n = {3: 0, 5: 150}.get(i, 30)                          # image 3: no proposals
        boxes = []
        for k in range(n):
            if gts and k % 3 != 2:
                x, y, w, h = gts[int(rng.integers(len(gts)))]
                s = [.05, .15, .4][k % 3]
                x, y = x + w * rng.normal(0, s), y + h * rng.normal(0, s)
                w, h = w * (1 + rng.normal(0, s)), h * (1 + rng.normal(0, s))
            else:
                x, y, w, h = rng.uniform(0, 1000), rng.uniform(0, 800), rng.uniform(10, 400), rng.uniform(10, 300)
            w, h = max(w, 2.0), max(h, 2.0)
            boxes.append([x * scale, y * scale, (x + w - 1) * scale, (y + h - 1) * scale])
        boxes = np.array(boxes, np.float32).reshape(-1, 4)
        objectness = rng.permutation(n).astype(np.float32) / max(n, 1)          # distinct: the order is unambiguous
        proposals.append({"size": list(size), "boxes": boxes.tolist(), "objectness": objectness.tolist()})
    return images, annotations, proposals


def main():
    _bare_packages(ref_shims.install())
    from maskrcnn_benchmark.data.datasets.evaluation.coco import coco_eval as ref
    from maskrcnn_benchmark.structures.bounding_box import BoxList as RefBoxList

    assert ref.__file__.startswith("/root/reference")
    images, annotations, proposals = make_inputs()
    dataset = _Dataset(images, annotations)
    predictions = []
    for p in proposals:
        box = RefBoxList(torch.tensor(p["boxes"], dtype=torch.float32).reshape(-1, 4), tuple(p["size"]), mode="xyxy")
        box.add_field("objectness", torch.tensor(p["objectness"], dtype=torch.float32))
        predictions.append(box)

    results = []
    for area in ("all", "small", "medium", "large", "96-128", "128-256", "256-512", "512-inf"):
        for limit in (100, 1000):
            r = ref.evaluate_box_proposals(predictions, dataset, area=area, limit=limit)
            assert r["num_pos"] > 0, "area range %s has no ground truth: change the sizes" % area
            results.append({"area": area, "limit": limit, "ar": r["ar"].item(), "recalls": r["recalls"].tolist(),
                            "thresholds": r["thresholds"].tolist(), "gt_overlaps": r["gt_overlaps"].tolist(),
                            "num_pos": int(r["num_pos"])})
            print("%-8s limit %4d: AR %.4f over %d ground truths" % (area, limit, results[-1]["ar"], r["num_pos"]))
    table = {}
    for limit in (100, 1000):
        for area, suffix in (("all", ""), ("small", "s"), ("medium", "m"), ("large", "l")):
            table["AR%s@%d" % (suffix, limit)] = ref.evaluate_box_proposals(predictions, dataset, area=area,
                                                                             limit=limit)["ar"].item()
    assert sorted(table) == sorted(ref.COCOResults.METRICS["box_proposal"])
    assert table["AR@100"] != table["AR@1000"], "the limit of 100 changes nothing: give an image more proposals"
    custom = ref.evaluate_box_proposals(predictions, dataset, thresholds=torch.tensor([.5, .7]), area="all", limit=None)
    out = {"images": images, "annotations": annotations, "category_ids": [1, 2], "proposals": proposals, "results": results,
           "box_proposal": table, "custom_thresholds_ar": custom["ar"].item()}
    path = os.path.join(HERE, "box_proposals.json")
    with open(path, "w") as f:
        json.dump(out, f)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
