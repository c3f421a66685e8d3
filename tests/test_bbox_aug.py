"""Test-time box augmentation (engine/bbox_aug.py, TEST.BBOX_AUG.*, BBoxAugCollator, PostProcessor(bbox_aug_enabled)).

Host side: the config node, the collator, the evaluation loader and the pass sequence (sizes, mirroring, order) with a
recording stub detector.  GPU side: the da_plain evaluation model of tests/test_model_gpu.py (192 x 320, seeded weights)
through `im_detect_bbox_aug` — the identity-only run equals plain evaluation exactly, and a flip + scale run gives exactly
the same detections through the device filter as through the Python loop."""
import json
import os

import numpy as np
import pytest
import torch

from golden.bbox_aug_stub import StubDetector, make_images

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")


def _cfg(*overrides):
    from da_detect_amd.config import cfg

    c = cfg.clone()
    c.merge_from_list(list(overrides))
    return c


# ------------------------------------------------------------------------------------------------------- host
def test_config_node_defaults_and_merging(tmp_path):
    from da_detect_amd.config import cfg

    aug = cfg.TEST.BBOX_AUG
    assert (aug.ENABLED, aug.H_FLIP, tuple(aug.SCALES), aug.MAX_SIZE, aug.SCALE_H_FLIP) == (False, False, (), 4000, False)
    path = str(tmp_path / "aug.yaml")
    with open(path, "w") as f:
        f.write("TEST:\n  BBOX_AUG:\n    ENABLED: True\n    H_FLIP: True\n    SCALES: (400, 600)\n    MAX_SIZE: 1000\n")
    c = cfg.clone()
    c.merge_from_file(path)
    assert c.TEST.BBOX_AUG.ENABLED is True and c.TEST.BBOX_AUG.H_FLIP is True and c.TEST.BBOX_AUG.SCALE_H_FLIP is False
    assert tuple(c.TEST.BBOX_AUG.SCALES) == (400, 600) and c.TEST.BBOX_AUG.MAX_SIZE == 1000
    assert c.TEST.DETECTIONS_PER_IMG == 100 and cfg.TEST.BBOX_AUG.ENABLED is False       # the rest and the global untouched
    c = _cfg("TEST.BBOX_AUG.ENABLED", "True", "TEST.BBOX_AUG.SCALES", "(400,)", "TEST.BBOX_AUG.SCALE_H_FLIP", True)
    assert c.TEST.BBOX_AUG.ENABLED is True and tuple(c.TEST.BBOX_AUG.SCALES) == (400,) and c.TEST.BBOX_AUG.SCALE_H_FLIP is True


def test_post_processor_factory_passes_the_switch():
    from da_detect_amd.modeling.roi_heads.box_head.inference import make_roi_box_post_processor

    assert make_roi_box_post_processor(_cfg()).bbox_aug_enabled is False
    assert make_roi_box_post_processor(_cfg("TEST.BBOX_AUG.ENABLED", True)).bbox_aug_enabled is True


def test_collator_leaves_samples_unbatched():
    from da_detect_amd.data.collate_batch import BBoxAugCollator

    a, b = object(), object()
    images, targets, ids = BBoxAugCollator()([(a, "ta", 3), (b, "tb", 5)])
    assert images == (a, b) and targets == ("ta", "tb") and ids == (3, 5)


def _write_coco(tmp, sizes):
    from PIL import Image

    rng = np.random.default_rng(3)
    root = os.path.join(tmp, "imgs")
    os.makedirs(root)
    images = []
    for i, (h, w) in enumerate(sizes):
        Image.fromarray(rng.integers(0, 255, (h, w, 3), dtype=np.uint8)).save(os.path.join(root, "im%d.png" % i))
        images.append({"id": 100 + i, "file_name": "im%d.png" % i, "height": h, "width": w})
    annos = [{"id": 1, "image_id": 100, "category_id": 24, "iscrowd": 0, "bbox": [5, 6, 20, 15], "area": 300}]
    ann = os.path.join(tmp, "ann.json")
    with open(ann, "w") as f:
        json.dump({"images": images, "annotations": annos, "categories": [{"id": 24, "name": "person"}]}, f)
    return ann, root


@pytest.mark.parametrize("enabled", [False, True])
def test_evaluation_loader_hands_out_raw_images_only_when_enabled(tmp_path, enabled):
    from PIL import Image

    from da_detect_amd.data.build import make_test_data_loader
    from da_detect_amd.data.datasets import COCODataset
    from da_detect_amd.data.transforms import build_transforms

    c = _cfg("TEST.BBOX_AUG.ENABLED", enabled, "TEST.IMS_PER_BATCH", 2, "DATALOADER.NUM_WORKERS", 0,
             "INPUT.MIN_SIZE_TEST", 32, "INPUT.MAX_SIZE_TEST", 64)
    ann, root = _write_coco(str(tmp_path), [(40, 80), (48, 60)])
    ds = COCODataset(ann, root, remove_images_without_annotations=False, transforms=build_transforms(c, is_train=False))
    images, targets, ids = next(iter(make_test_data_loader(c, ds)))
    assert list(ids) == [0, 1] and len(targets) == 2
    if enabled:
        assert isinstance(images, tuple) and all(isinstance(im, Image.Image) for im in images)
        assert [im.size for im in images] == [(80, 40), (60, 48)]          # untransformed
    else:
        assert tuple(images.tensors.shape) == (2, 3, 32, 64) and images.tensors.dtype == torch.float32


# (w, h) of the two images of make_images() — 100 x 60 and 90 x 72 — per pass; worked out by hand from the reference's
# Resize rule (transforms.py:41-62): the shorter side goes to the scale, the longer one is truncated; scale 120 would
# stretch the first image to 200 > MAX_SIZE 150, so its shorter side becomes round(150 * 60 / 100) = 90; the second
# image reaches exactly 150, which is not above the cap
_IDENTITY = [(80, 48), (60, 48)]
_SCALE_64 = [(106, 64), (80, 64)]
_SCALE_120 = [(150, 90), (150, 120)]


@pytest.mark.parametrize("h_flip", [False, True])
@pytest.mark.parametrize("scale_h_flip", [False, True])
def test_pass_sequence(h_flip, scale_h_flip):
    """sizes per pass, which passes see the mirror image, and the order identity -> flip -> scale -> scale + flip"""
    from PIL import Image

    from da_detect_amd.engine.bbox_aug import im_detect_bbox_aug
    from da_detect_amd.structures.bounding_box import BoxList

    c = _cfg("TEST.BBOX_AUG.ENABLED", True, "TEST.BBOX_AUG.H_FLIP", h_flip, "TEST.BBOX_AUG.SCALE_H_FLIP", scale_h_flip,
             "TEST.BBOX_AUG.SCALES", (64, 120), "TEST.BBOX_AUG.MAX_SIZE", 150, "INPUT.MIN_SIZE_TEST", 48,
             "INPUT.MAX_SIZE_TEST", 96, "DATALOADER.SIZE_DIVISIBILITY", 32, "MODEL.ROI_BOX_HEAD.NUM_CLASSES", 4)
    model = StubDetector(lambda boxes, size: BoxList(boxes, size, mode="xyxy"), num_classes=4, empty=True)
    model.cfg = c
    images = [Image.fromarray(im) for im in make_images()]
    out = im_detect_bbox_aug(model, images, torch.device("cpu"))
    want = [(_IDENTITY, False)] + ([(_IDENTITY, True)] if h_flip else [])
    for sizes in (_SCALE_64, _SCALE_120):
        want += [(sizes, False)] + ([(sizes, True)] if scale_h_flip else [])
    assert len(model.calls) == len(want)
    for call, (sizes, mirrored) in zip(model.calls, want):
        assert call["sizes"] == sizes
        assert call["left_brighter"] == [not mirrored] * 2          # the images' left halves are the bright ones
        assert call["padded"] == tuple(-(-max(s[k] for s in sizes) // 32) * 32 for k in (1, 0))
    assert len(out) == 2 and all(len(o) == 0 for o in out)
    assert [o.size for o in out] == _IDENTITY and all(o.get_field("labels").dtype == torch.int64 for o in out)


def test_inference_signatures_keep_their_defaults():
    import inspect

    from da_detect_amd.engine import inference as I

    p = inspect.signature(I.compute_on_dataset).parameters
    assert list(p)[:3] == ["model", "data_loader", "device"] and p["bbox_aug"].default is False and p["timer"].default is None
    assert inspect.signature(I.inference).parameters["bbox_aug"].default is False


def test_inference_takes_the_passes_from_an_augmentation_loader(tmp_path):
    """a loader built with TEST.BBOX_AUG.ENABLED carries the BBoxAugCollator: `inference` then runs the augmentation
    passes without a `bbox_aug` argument (what the unchanged tools/test_net_da.py relies on); a plain loader does not"""
    from da_detect_amd.data.build import make_test_data_loader
    from da_detect_amd.data.datasets import COCODataset
    from da_detect_amd.data.transforms import build_transforms
    from da_detect_amd.engine.inference import inference
    from da_detect_amd.structures.bounding_box import BoxList

    ann, root = _write_coco(str(tmp_path), [(40, 80), (48, 60)])
    calls = {}
    for enabled in (True, False):
        c = _cfg("TEST.BBOX_AUG.ENABLED", enabled, "TEST.BBOX_AUG.H_FLIP", True, "TEST.IMS_PER_BATCH", 2,
                 "DATALOADER.NUM_WORKERS", 0, "INPUT.MIN_SIZE_TEST", 32, "INPUT.MAX_SIZE_TEST", 64,
                 "MODEL.ROI_BOX_HEAD.NUM_CLASSES", 4)
        ds = COCODataset(ann, root, remove_images_without_annotations=False, transforms=build_transforms(c, is_train=False))
        model = StubDetector(lambda boxes, size: BoxList(boxes, size, mode="xyxy"), num_classes=4, empty=True)
        model.cfg = c
        if not enabled:     # plain evaluation hands the model's (filtered) output on: give the empty lists their labels
            model = _Labelled(model)
        records = inference(model, make_test_data_loader(c, ds), "tiny", device="cpu")
        assert records == []
        calls[enabled] = (model.inner if not enabled else model).calls
    assert len(calls[True]) == 2 and len(calls[False]) == 1          # identity + flip against the one plain pass
    assert calls[True][0]["sizes"] == calls[True][1]["sizes"] == calls[False][0]["sizes"] == [(64, 32), (40, 32)]


class _Labelled(object):
    """a detector whose empty BoxLists carry a `labels` field, as a post-processor's output does"""

    def __init__(self, inner):
        self.inner = inner

    def eval(self):
        return self

    def __call__(self, images):
        out = self.inner(images)
        for o in out:
            o.add_field("labels", torch.zeros((0,), dtype=torch.int64))
        return out


def test_compat_aliases_the_module():
    import importlib

    from da_detect_amd import compat

    compat.install()
    mod = importlib.import_module("maskrcnn_benchmark.engine.bbox_aug")
    assert all(hasattr(mod, n) for n in ("im_detect_bbox_aug", "im_detect_bbox", "im_detect_bbox_hflip", "im_detect_bbox_scale"))


# -------------------------------------------------------------------------------------------------------- GPU
def _eval_model(device, *overrides):
    from da_detect_amd.modeling.detector import build_detection_model
    from golden.cases import case_cfg
    from golden.fill import fill_state_dict

    z = np.load(os.path.join(GOLD, "eval_da_plain.npz"))
    c = case_cfg("da_plain")
    c.merge_from_list(["INPUT.MIN_SIZE_TEST", int(z["H"]), "INPUT.MAX_SIZE_TEST", int(z["W"])] + list(overrides))
    model = build_detection_model(c)
    model.load_state_dict(fill_state_dict(model.state_dict(), int(z["seed"])))
    return c, model.to(device).eval(), int(z["H"]), int(z["W"])


def _pil_images(H, W, n=2):
    from PIL import Image

    rng = np.random.default_rng(5)
    out = []
    for _ in range(n):
        im = rng.integers(0, 256, (H // 8, W // 8, 3), dtype=np.uint8).repeat(8, 0).repeat(8, 1)      # blocky: some structure
        out.append(Image.fromarray(im))
    return out


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.size == y.size
        assert torch.equal(x.get_field("labels"), y.get_field("labels"))
        assert torch.equal(x.get_field("scores"), y.get_field("scores")) and torch.equal(x.bbox, y.bbox)


@pytest.mark.gpu
def test_identity_only_augmentation_equals_plain_evaluation(device):
    """no flip, no scales: the identity pass is filtered alone, which is plain evaluation"""
    from da_detect_amd.data.transforms import build_transforms
    from da_detect_amd.engine.bbox_aug import im_detect_bbox_aug
    from da_detect_amd.structures.image_list import to_image_list

    c, model, H, W = _eval_model(device, "MODEL.ROI_HEADS.SCORE_THRESH", 0.02)
    images = _pil_images(H, W)
    tf = build_transforms(c, is_train=False)
    with torch.no_grad():
        plain = model(to_image_list([tf(im, None)[0] for im in images], c.DATALOADER.SIZE_DIVISIBILITY).to(device))
    c_aug, model_aug, _, _ = _eval_model(device, "MODEL.ROI_HEADS.SCORE_THRESH", 0.02, "TEST.BBOX_AUG.ENABLED", True)
    with torch.no_grad():
        aug = im_detect_bbox_aug(model_aug, images, device)
    assert sum(len(p) for p in plain) > 0
    _same(aug, plain)


@pytest.mark.gpu
def test_flip_and_scale_device_filter_equals_loop(device, monkeypatch):
    """H_FLIP plus one scale: the switch at 1 equals the switch at 0 exactly; detections inside the image; the cut rule"""
    from da_detect_amd.engine.bbox_aug import im_detect_bbox_aug

    k = 20
    c, model, H, W = _eval_model(device, "MODEL.ROI_HEADS.SCORE_THRESH", 0.02, "TEST.BBOX_AUG.ENABLED", True,
                                 "TEST.BBOX_AUG.H_FLIP", True, "TEST.BBOX_AUG.SCALES", (160,), "TEST.DETECTIONS_PER_IMG", k,
                                 "MODEL.ROI_HEADS.DETECTIONS_PER_IMG", k)
    images = _pil_images(H, W)
    results = {}
    for switch in ("1", "0"):
        monkeypatch.setenv("DADET_DEVICE_POSTPROCESS", switch)
        with torch.no_grad():
            results[switch] = im_detect_bbox_aug(model, images, device)
    _same(results["1"], results["0"])
    assert sum(len(r) for r in results["1"]) > 0
    for r in results["1"]:
        assert r.size == (W, H)
        b, s = r.bbox, r.get_field("scores")
        assert len(r) == 0 or (float(b[:, 0::2].min()) >= 0 and float(b[:, 0::2].max()) <= W - 1 and
                               float(b[:, 1::2].min()) >= 0 and float(b[:, 1::2].max()) <= H - 1)
        if len(r) > k:      # more than k only through ties at the cut value: the k-th largest score is the smallest kept
            kth = torch.sort(s, descending=True).values[k - 1]
            assert float(s.min()) == float(kth)
        assert bool((s > 0.02).all())


@pytest.mark.gpu
def test_augmentation_matches_reference_golden(device):
    """the reference's im_detect_bbox_aug + post-processor with the same stand-in detector on the same two images
    (tests/golden/make_golden_bbox_aug.py -> bbox_aug_stub.npz): labels and scores equal, boxes within 1e-4 (BoxList
    resize arithmetic), and what every pass was given within 1e-4 relative — resize, flip, normalisation, pass order"""
    import ast

    from PIL import Image

    from da_detect_amd.engine.bbox_aug import im_detect_bbox_aug
    from da_detect_amd.structures.bounding_box import BoxList

    z = np.load(os.path.join(GOLD, "bbox_aug_stub.npz"))
    c = _cfg(*ast.literal_eval(str(z["overrides"])))
    model = StubDetector(lambda boxes, size: BoxList(boxes, size, mode="xyxy"), num_classes=4)
    model.cfg = c
    images = [Image.fromarray(z["image/%d" % i]) for i in range(2)]
    for a, b in zip(make_images(), images):
        assert np.array_equal(a, np.array(b))
    with torch.no_grad():
        dets = im_detect_bbox_aug(model, images, device)
    assert len(model.calls) == int(z["passes"]) == 6
    for p, call in enumerate(model.calls):
        assert np.array_equal(np.array(call["sizes"]), z["pass/%d/sizes" % p])
        assert tuple(call["padded"]) == tuple(z["pass/%d/padded" % p])
        assert call["left_brighter"] == z["pass/%d/left_brighter" % p].tolist()
        np.testing.assert_allclose(call["sums"], z["pass/%d/sums" % p], rtol=1e-4)
        np.testing.assert_allclose(call["probes"], z["pass/%d/probes" % p], rtol=1e-4)
    for i, d in enumerate(dets):
        assert d.bbox.is_cuda and d.size == tuple(z["det/%d/size" % i])
        assert np.array_equal(d.get_field("labels").cpu().numpy(), z["det/%d/labels" % i])
        assert np.array_equal(d.get_field("scores").cpu().numpy(), z["det/%d/scores" % i])
        np.testing.assert_allclose(d.bbox.cpu().numpy(), z["det/%d/boxes" % i], rtol=0, atol=1e-4)
