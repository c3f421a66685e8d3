"""COCO-style and PASCAL VOC detection datasets with a domain flag (reference: maskrcnn_benchmark/data/datasets/coco.py:44-124,
data/datasets/voc.py and data/build.py:23-63 `Dataset_triplet`).  The annotation file is read with the json module (pycocotools /
torchvision.datasets.CocoDetection are not needed for bounding boxes); segmentation masks and keypoints are outside the
DA Faster R-CNN path."""
import collections
import copy
import json
import os
import xml.etree.ElementTree as ET

import numpy as np
import torch

from ..structures.bounding_box import BoxList

MIN_KEYPOINTS_PER_IMAGE = 10

# what a `decode_to_tensor=True` dataset with transforms puts into a sample's image slot: the decoded pixels (uint8 [H,W,3],
# CPU) and the decisions its transforms WOULD apply, decision = ((out_h, out_w), flip) — with a vertical flip or a colour jitter
# in the chain ((out_h, out_w), flip, vertical flip, jitter operators), data/transforms.py draw_decisions — data/device_prep.py applies them
RawImage = collections.namedtuple("RawImage", ["pixels", "decision"])


def raw_image(img, transforms):
    """PIL image -> the image slot of a `decode_to_tensor=True` sample.  The random decisions are drawn here, where the
    host chain draws them (inside __getitem__, so inside the loader's worker with its seeding) and in its order; with
    `transforms=None` the slot holds the pixels alone."""
    pixels = torch.from_numpy(np.array(img, dtype=np.uint8))
    if transforms is None:
        return pixels
    from .transforms import draw_decisions

    return RawImage(pixels, draw_decisions(transforms, img.size))


def has_valid_annotation(anno):
    """coco.py:21-41 for box-only annotations: at least one box that is not (nearly) degenerate"""
    if len(anno) == 0:
        return False
    if all(any(o <= 1 for o in obj["bbox"][2:]) for obj in anno):
        return False
    return True


class COCODataset(torch.utils.data.Dataset):
    def __init__(self, ann_file, root, remove_images_without_annotations, transforms=None, is_source=True,
                 decode_to_tensor=False):
        if isinstance(ann_file, dict):               # already loaded (data/cityscapes.py builds it from the id maps)
            data = ann_file
        else:
            with open(ann_file) as f:
                data = json.load(f)
        self.root = root
        self.imgs = {im["id"]: im for im in data["images"]}
        self.anns_of = {}
        for a in data.get("annotations", []):
            self.anns_of.setdefault(a["image_id"], []).append(a)
        self.ids = sorted(self.imgs.keys())
        if remove_images_without_annotations:
            self.ids = [i for i in self.ids if has_valid_annotation(self.anns_of.get(i, []))]
        cat_ids = sorted(c["id"] for c in data.get("categories", []))
        self.category_names = {c["id"]: c.get("name", str(c["id"])) for c in data.get("categories", [])}
        self.json_category_id_to_contiguous_id = {v: i + 1 for i, v in enumerate(cat_ids)}
        self.contiguous_category_id_to_json_id = {v: k for k, v in self.json_category_id_to_contiguous_id.items()}
        self.id_to_img_map = {k: v for k, v in enumerate(self.ids)}
        self._transforms = transforms
        self.is_source = is_source
        self.decode_to_tensor = decode_to_tensor     # True: return uint8 [H,W,3] for data/device_prep.py

    def __len__(self):
        return len(self.ids)

    def _load_image(self, img_id):
        from PIL import Image

        return Image.open(os.path.join(self.root, self.imgs[img_id]["file_name"])).convert("RGB")

    def __getitem__(self, idx):
        img_id = self.ids[idx]
        img = self._load_image(img_id)
        anno = [o for o in self.anns_of.get(img_id, []) if o.get("iscrowd", 0) == 0]
        boxes = torch.as_tensor([o["bbox"] for o in anno], dtype=torch.float32).reshape(-1, 4)
        target = BoxList(boxes, img.size, mode="xywh").convert("xyxy")
        classes = torch.tensor([self.json_category_id_to_contiguous_id[o["category_id"]] for o in anno],
                               dtype=torch.int64)
        target.add_field("labels", classes)
        target.add_field("is_source", torch.full_like(classes, bool(self.is_source), dtype=torch.bool))
        target = target.clip_to_image(remove_empty=True)
        if self.decode_to_tensor:
            return raw_image(img, self._transforms), target, idx
        if self._transforms is not None:
            img, target = self._transforms(img, target)
        return img, target, idx

    def get_img_info(self, index):
        return self.imgs[self.id_to_img_map[index]]

    def get_groundtruth(self, index):
        """every annotation of the image as the VOC scorer wants it (data/evaluation/voc): xyxy boxes with `labels` and
        `difficult` = iscrowd (VOC's "neither right nor wrong to find" is what COCO means by a crowd region)"""
        info = self.get_img_info(index)
        anno = self.anns_of.get(self.id_to_img_map[index], [])
        boxes = torch.as_tensor([o["bbox"] for o in anno], dtype=torch.float32).reshape(-1, 4)
        target = BoxList(boxes, (info["width"], info["height"]), mode="xywh").convert("xyxy")
        target.add_field("labels", torch.tensor([self.json_category_id_to_contiguous_id[o["category_id"]] for o in anno],
                                                dtype=torch.int64))
        target.add_field("difficult", torch.tensor([bool(o.get("iscrowd", 0)) for o in anno], dtype=torch.bool))
        return target

    def map_class_id_to_class_name(self, class_id):
        if class_id == 0:
            return "__background__"
        json_id = self.contiguous_category_id_to_json_id[class_id]
        return self.category_names.get(json_id, str(json_id))


class PascalVOCDataset(torch.utils.data.Dataset):
    """a dataset in PASCAL VOC layout: Annotations/<id>.xml, ImageSets/Main/<split>.txt, JPEGImages/<id>.jpg.  `classes`
    replaces the twenty VOC names (background first; Cityscapes in VOC layout has eight); `use_difficult` keeps the objects
    marked difficult (evaluation needs them: they are neither hits nor misses), training drops them."""

    CLASSES = ("__background__ ", "aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow",
               "diningtable", "dog", "horse", "motorbike", "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor")

    def __init__(self, data_dir, split, use_difficult=False, transforms=None, is_source=True, decode_to_tensor=False,
                 classes=None):
        self.root = data_dir
        self.image_set = split
        self.keep_difficult = use_difficult
        self._transforms = transforms
        self.is_source = is_source
        self.decode_to_tensor = decode_to_tensor     # True: return uint8 [H,W,3] for data/device_prep.py
        self._annopath = os.path.join(self.root, "Annotations", "%s.xml")
        self._imgpath = os.path.join(self.root, "JPEGImages", "%s.jpg")
        self._imgsetpath = os.path.join(self.root, "ImageSets", "Main", "%s.txt")
        with open(self._imgsetpath % self.image_set) as f:
            self.ids = [line.strip() for line in f if line.strip()]
        self.id_to_img_map = dict(enumerate(self.ids))
        if classes is not None:
            self.CLASSES = tuple(classes)
        self.class_to_ind = {name: i for i, name in enumerate(self.CLASSES)}

    def __len__(self):
        return len(self.ids)

    def __getitem__(self, index):
        from PIL import Image

        img = Image.open(self._imgpath % self.ids[index]).convert("RGB")
        target = self.get_groundtruth(index)
        labels = target.get_field("labels")
        target.add_field("is_source", torch.full_like(labels, bool(self.is_source), dtype=torch.bool))
        target = target.clip_to_image(remove_empty=True)
        if self.decode_to_tensor:
            return raw_image(img, self._transforms), target, index
        if self._transforms is not None:
            img, target = self._transforms(img, target)
        return img, target, index

    def _root_of(self, index):
        return ET.parse(self._annopath % self.ids[index]).getroot()

    @staticmethod
    def _size(anno):
        size = anno.find("size")
        return int(size.find("height").text), int(size.find("width").text)

    def get_groundtruth(self, index):
        anno = self._preprocess_annotation(self._root_of(index))
        height, width = anno["im_info"]
        target = BoxList(anno["boxes"], (width, height), mode="xyxy")
        target.add_field("labels", anno["labels"])
        target.add_field("difficult", anno["difficult"])
        return target

    def _preprocess_annotation(self, target):
        """VOC pixel indices are 1-based: every coordinate loses 1"""
        boxes, labels, difficult = [], [], []
        for obj in target.iter("object"):
            hard = obj.find("difficult")
            hard = hard is not None and int(hard.text) == 1
            if hard and not self.keep_difficult:
                continue
            bb = obj.find("bndbox")
            boxes.append([int(bb.find(k).text) - 1 for k in ("xmin", "ymin", "xmax", "ymax")])
            labels.append(self.class_to_ind[obj.find("name").text.lower().strip()])
            difficult.append(hard)
        return {"boxes": torch.tensor(boxes, dtype=torch.float32).reshape(-1, 4),
                "labels": torch.tensor(labels, dtype=torch.int64), "difficult": torch.tensor(difficult, dtype=torch.bool),
                "im_info": self._size(target)}

    def get_img_info(self, index):
        height, width = self._size(self._root_of(index))
        return {"height": height, "width": width}

    def map_class_id_to_class_name(self, class_id):
        return self.CLASSES[class_id]


class ConcatDataset(torch.utils.data.ConcatDataset):
    """concatenation that still answers get_img_info (reference: data/datasets/concat_dataset.py:7-23)"""

    def get_img_info(self, idx):
        import bisect

        which = bisect.bisect_right(self.cumulative_sizes, idx)
        return self.datasets[which].get_img_info(idx if which == 0 else idx - self.cumulative_sizes[which - 1])


class TripletDataset(torch.utils.data.Dataset):
    """index-aligned (source, target, auxiliary) samples; the target / auxiliary images are paired with a COPY of the
    source annotations carrying their own domain flag — build.py:34-46 (the datasets are renderings of the same
    scenes: Cityscapes, its foggy and its rainy version)"""

    def __init__(self, datasets):
        assert len(datasets) == 3
        self.dataset_s, self.dataset_p, self.dataset_n = datasets

    def __len__(self):
        return len(self.dataset_s)

    @staticmethod
    def _with_domain(target_s, target_other):
        t = copy.deepcopy(target_s)
        t.add_field("is_source", copy.deepcopy(target_other.get_field("is_source")))
        return t

    def __getitem__(self, index):
        img_s, target_s, i1 = self.dataset_s[index]
        img_p, target_p, i2 = self.dataset_p[index]
        img_n, target_n, i3 = self.dataset_n[index]
        return (img_s, target_s, img_p, self._with_domain(target_s, target_p), img_n,
                self._with_domain(target_s, target_n), i1, i2, i3)

    def get_img_info(self, index):
        return self.dataset_s.get_img_info(index)


Dataset_triplet = TripletDataset      # the reference's name (data/build.py:23)


# ------------------------------------------------------------------------------- the synthesised rainy domain (data/rain.py)
class RainImage(RawImage):
    """the image slot of a `decode_to_tensor=True` sample of RainyDataset: a RawImage of the SOURCE pixels that also says
    which rain mask to blend into them and how (data/rain.py RainPlan) — data/device_prep.py synthesises the rainy image on
    the device before it prepares the batch.  In an aligned triplet `pixels` is the source sample's own tensor."""

    def __new__(cls, pixels, decision, mask_index, plan):
        self = super(RainImage, cls).__new__(cls, pixels, decision)
        self.mask_index, self.plan = mask_index, plan
        return self

    def __reduce__(self):
        return RainImage, (self.pixels, self.decision, self.mask_index, self.plan)


def finish_sample(dataset, img, target, index):
    """what COCODataset / PascalVOCDataset.__getitem__ do with a loaded (PIL image, target): a raw sample, or its transforms"""
    if dataset.decode_to_tensor:
        return raw_image(img, dataset._transforms), target, index
    if dataset._transforms is not None:
        img, target = dataset._transforms(img, target)
    return img, target, index


class RainyDataset(torch.utils.data.Dataset):
    """the rainy rendering of `source`'s images, synthesised per sample instead of read from disk (data/rain.py): same
    length, annotations and get_img_info, is_source False.  Every sample draws, from Python's `random` and before the
    decisions of its transforms: the rain mask (randrange) and the seed (getrandbits(32)) of the numpy RandomState its rain
    plan comes from — so every epoch sees fresh rain.  Host chain: the composited PIL image goes through the source's
    transforms.  decode_to_tensor: the image slot is a RainImage (source pixels + mask index + plan + decisions).
    `source` is a COCODataset / PascalVOCDataset; its transforms and decode_to_tensor switch are this dataset's.  The
    untransformed samples come from a shallow copy of it without transforms (`load`)."""

    is_source = False

    def __init__(self, source, masks):
        self.source, self.masks = source, masks
        self._plain = copy.copy(source)
        self._plain._transforms, self._plain.decode_to_tensor = None, False

    _transforms = property(lambda self: self.source._transforms,
                           lambda self, value: setattr(self.source, "_transforms", value))
    decode_to_tensor = property(lambda self: self.source.decode_to_tensor,
                                lambda self, value: setattr(self.source, "decode_to_tensor", value))

    def __len__(self):
        return len(self.source)

    def get_img_info(self, index):
        return self.source.get_img_info(index)

    def __getattr__(self, name):            # id maps, category tables, get_groundtruth: the source's
        if name in ("source", "masks", "_plain") or name.startswith("__"):
            raise AttributeError(name)
        return getattr(self.source, name)

    def load(self, index):
        """-> (PIL image, target) of the source sample, before any transform, the domain flag still the source's"""
        img, target, _ = self._plain[index]
        return img, target

    def rainy_sample(self, img, target, index, pixels=None):
        """img, target: `load(index)` (neither is modified); pixels: img as a uint8 tensor when the caller has it already
        (the aligned triplet's source sample)"""
        import random

        from . import rain
        from .transforms import draw_decisions

        mask_index = random.randrange(len(self.masks))
        plan = rain.draw_rain_plan(np.random.RandomState(random.getrandbits(32)), img.size[0], img.size[1])
        target = copy.deepcopy(target)
        target.add_field("is_source", torch.zeros_like(target.get_field("labels"), dtype=torch.bool))
        if self.decode_to_tensor:
            if pixels is None:
                pixels = torch.from_numpy(np.array(img, dtype=np.uint8))
            return RainImage(pixels, draw_decisions(self._transforms, img.size), mask_index, plan), target, index
        from PIL import Image

        img = Image.fromarray(rain.synthesize_host(np.asarray(img, dtype=np.uint8), self.masks.host_mask(mask_index, img.size),
                                                   plan))
        if self._transforms is not None:
            img, target = self._transforms(img, target)
        return img, target, index

    def __getitem__(self, index):
        img, target = self.load(index)
        return self.rainy_sample(img, target, index)


class RainTripletDataset(TripletDataset):
    """TripletDataset whose auxiliary is a RainyDataset over the source dataset ITSELF: the source image is decoded once per
    triplet — the source sample is finished from it, the rainy sample drawn from it after the target sample, where a third
    dataset's sample would draw; as raw samples the two share one pixel tensor (one upload)."""

    def __init__(self, datasets):
        super(RainTripletDataset, self).__init__(datasets)
        assert isinstance(self.dataset_n, RainyDataset) and self.dataset_n.source is self.dataset_s

    def __getitem__(self, index):
        decoded, plain = self.dataset_n.load(index)
        img_s, target_s, i1 = finish_sample(self.dataset_s, decoded, plain, index)
        img_p, target_p, i2 = self.dataset_p[index]
        img_n, target_n, i3 = self.dataset_n.rainy_sample(decoded, plain, index,
                                                          img_s.pixels if isinstance(img_s, RawImage) else None)
        return (img_s, target_s, img_p, self._with_domain(target_s, target_p), img_n,
                self._with_domain(target_s, target_n), i1, i2, i3)
