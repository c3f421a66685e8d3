"""Golden vectors for test-time box augmentation — runs ONLY in the authoring container (needs /root/reference).

Runs the reference's own `im_detect_bbox_aug` and post-processor (the VENDORED tree tools/cityscapes/maskrcnn_benchmark:
engine/bbox_aug.py, modeling/roi_heads/box_head/inference.py, data/transforms, structures) on two small seeded images
with the stand-in detector of tests/golden/bbox_aug_stub.py and stores, in tests/golden/bbox_aug_stub.npz, the two uint8
input images, what the detector was given in every pass (sizes, sums, probe pixels) and the final boxes, scores and labels.

What is substituted, all of it here and none of it in ref_shims.py or the reference:
  * the vendored tree's package __init__ files pull in its datasets, its JIT-built extension and apex; the packages are
    registered as bare namespaces over the vendored directories, so only the modules named above are executed, and
    `maskrcnn_benchmark.layers.nms` is the reference's compiled CPU NMS (oracle/_ref, built from the reference's csrc);
  * `torchvision.transforms` is not installed: a minimal Pillow-based stand-in for the five functions the vendored
    transforms and bbox_aug.py use — resize (bilinear), hflip, to_tensor, normalize, Compose (with the ToTensor and
    RandomHorizontalFlip classes built on them) — written from torchvision's documented behaviour for PIL images.

The generator asserts that no pairwise IoU of same-class candidates lies within 1e-6 of the NMS threshold, so the
reference's CPU tie rule (>=) and its CUDA one (>) give the same detections and the fixture holds for either, and that no
two candidates of a class share a score (the reference's CPU NMS ranks with an unstable sort).

    python tests/golden/make_golden_bbox_aug.py
"""
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
from bbox_aug_stub import StubDetector, make_images  # noqa: E402

VENDORED = "/root/reference/tools/cityscapes/maskrcnn_benchmark"
OVERRIDES = ["TEST.BBOX_AUG.ENABLED", True, "TEST.BBOX_AUG.H_FLIP", True, "TEST.BBOX_AUG.SCALES", (64, 120),
             "TEST.BBOX_AUG.MAX_SIZE", 150, "TEST.BBOX_AUG.SCALE_H_FLIP", True, "INPUT.MIN_SIZE_TEST", 48,
             "INPUT.MAX_SIZE_TEST", 96, "DATALOADER.SIZE_DIVISIBILITY", 32, "MODEL.ROI_BOX_HEAD.NUM_CLASSES", 4,
             "MODEL.ROI_HEADS.SCORE_THRESH", 0.05, "MODEL.ROI_HEADS.NMS", 0.5, "MODEL.ROI_HEADS.DETECTIONS_PER_IMG", 30]


def _torchvision_stand_in():
    from PIL import Image

    def resize(img, size, interpolation=Image.BILINEAR):
        h, w = size
        return img.resize((w, h), interpolation)

    def hflip(img):
        return img.transpose(Image.FLIP_LEFT_RIGHT)

    def to_tensor(img):
        a = np.array(img, dtype=np.uint8)
        a = a[:, :, None] if a.ndim == 2 else a
        return torch.from_numpy(np.ascontiguousarray(a)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)

    def normalize(t, mean, std):
        mean = torch.as_tensor(mean, dtype=t.dtype).view(-1, 1, 1)
        std = torch.as_tensor(std, dtype=t.dtype).view(-1, 1, 1)
        return (t - mean) / std

    class Compose(object):
        def __init__(self, transforms):
            self.transforms = transforms

        def __call__(self, img):
            for t in self.transforms:
                img = t(img)
            return img

    class ToTensor(object):
        def __call__(self, img):
            return to_tensor(img)

    class RandomHorizontalFlip(object):
        def __init__(self, p=0.5):
            self.p = p

        def __call__(self, img):
            return hflip(img) if torch.rand(1).item() < self.p else img

    tv, tt, tf = (types.ModuleType(n) for n in ("torchvision", "torchvision.transforms", "torchvision.transforms.functional"))
    tf.resize, tf.hflip, tf.to_tensor, tf.normalize = resize, hflip, to_tensor, normalize
    tt.Compose, tt.ToTensor, tt.RandomHorizontalFlip, tt.functional = Compose, ToTensor, RandomHorizontalFlip, tf
    tv.transforms = tt
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tt, "torchvision.transforms.functional": tf})


def _vendored_tree(ref_c):
    """maskrcnn_benchmark = the vendored tree, its packages as bare namespaces (see the module docstring)"""
    for name in [n for n in sys.modules if n == "maskrcnn_benchmark" or n.startswith("maskrcnn_benchmark.")]:
        del sys.modules[name]
    for sub in ("", ".data", ".structures", ".engine", ".modeling", ".modeling.roi_heads", ".modeling.roi_heads.box_head"):
        m = types.ModuleType("maskrcnn_benchmark" + sub)
        m.__path__ = [os.path.join(VENDORED, *[p for p in sub.split(".") if p])]
        sys.modules[m.__name__] = m
    layers = types.ModuleType("maskrcnn_benchmark.layers")
    layers.nms = ref_c.nms
    sys.modules["maskrcnn_benchmark.layers"] = layers
    sys.modules["maskrcnn_benchmark._C"] = ref_c


def _assert_no_iou_near_threshold(boxlist, num_classes, score_thresh, nms_thresh):
    b = boxlist.bbox.reshape(-1, num_classes, 4).double()
    s = boxlist.get_field("scores").reshape(-1, num_classes)
    for j in range(1, num_classes):
        x = b[s[:, j] > score_thresh, j]
        cand = s[s[:, j] > score_thresh, j]
        assert len(torch.unique(cand)) == len(cand), "two candidates of a class share a score: change the seed"
        area = (x[:, 2] - x[:, 0] + 1) * (x[:, 3] - x[:, 1] + 1)
        wh = (torch.min(x[:, None, 2:], x[:, 2:]) - torch.max(x[:, None, :2], x[:, :2]) + 1).clamp(min=0)
        inter = wh[..., 0] * wh[..., 1]
        iou = inter / (area[:, None] + area - inter)
        assert float((iou - nms_thresh).abs().min()) > 1e-6, "an IoU within 1e-6 of the NMS threshold: change the seed"


def main():
    ref_c = ref_shims.install()
    _torchvision_stand_in()
    _vendored_tree(ref_c)
    from PIL import Image

    import maskrcnn_benchmark.engine.bbox_aug as ref_aug
    from maskrcnn_benchmark.config import cfg as ref_cfg
    from maskrcnn_benchmark.modeling.roi_heads.box_head import inference as ref_post
    from maskrcnn_benchmark.structures.bounding_box import BoxList as RefBoxList

    assert ref_aug.__file__.startswith(VENDORED) and ref_post.__file__.startswith(VENDORED)
    ref_cfg.merge_from_list(OVERRIDES)      # bbox_aug.py reads the package-level cfg
    arrays = make_images()
    images = [Image.fromarray(a) for a in arrays]
    model = StubDetector(lambda boxes, size: RefBoxList(boxes, size, mode="xyxy"), num_classes=4)

    # the merged, unfiltered lists once more, for the near-threshold check (filter_results is wrapped, not changed)
    merged = []
    real_filter = ref_post.PostProcessor.filter_results

    def spy(self, boxlist, num_classes):
        merged.append(boxlist)
        return real_filter(self, boxlist, num_classes)

    ref_post.PostProcessor.filter_results = spy
    try:
        with torch.no_grad():
            dets = ref_aug.im_detect_bbox_aug(model, images, torch.device("cpu"))
    finally:
        ref_post.PostProcessor.filter_results = real_filter
    for boxlist in merged:
        _assert_no_iou_near_threshold(boxlist, 4, 0.05, 0.5)

    out = {"overrides": np.array(repr(OVERRIDES)), "passes": np.int64(len(model.calls))}
    for i, a in enumerate(arrays):
        out["image/%d" % i] = a
    for p, call in enumerate(model.calls):
        out["pass/%d/sizes" % p] = np.array(call["sizes"], np.int64)
        out["pass/%d/padded" % p] = np.array(call["padded"], np.int64)
        out["pass/%d/sums" % p] = np.array(call["sums"], np.float64)
        out["pass/%d/probes" % p] = np.array(call["probes"], np.float64)
        out["pass/%d/left_brighter" % p] = np.array(call["left_brighter"], np.bool_)
    for i, d in enumerate(dets):
        assert 0 < len(d) and len(merged[i]) // 4 == 6 * model.rows
        kept = len(d) / float((merged[i].get_field("scores").reshape(-1, 4)[:, 1:] > 0.05).sum())
        print("image %d: %d detections of %d merged rows (%.0f%% of the candidates)" % (i, len(d), len(merged[i]) // 4,
                                                                                      100 * kept))
        out["det/%d/size" % i] = np.array(d.size, np.int64)
        out["det/%d/boxes" % i] = d.bbox.numpy()
        out["det/%d/scores" % i] = d.get_field("scores").numpy()
        out["det/%d/labels" % i] = d.get_field("labels").numpy()
    path = os.path.join(HERE, "bbox_aug_stub.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d passes)" % (path, os.path.getsize(path), len(model.calls)))


if __name__ == "__main__":
    main()
