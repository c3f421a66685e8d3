"""The device input pipeline on the GPU: the batched preparation kernel (csrc/image.hip prepare_batch_kernel, one launch
per batch, 16 x 64 output tiles, input rows walked in chunks of 64) against Pillow / oracle.image_ref.preprocess bit for
bit, the device_prep loaders against the host loaders, test-time augmentation from uint8 tensors against the PIL path,
and tools/train_net_da.py --device-prep end to end."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from golden.bbox_aug_stub import StubDetector, make_images
from test_data_pipeline import _image, _write_coco

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
pytest.importorskip("PIL")
from PIL import Image  # noqa: E402

pytestmark = pytest.mark.gpu
TILE_H, TILE_W = 16, 64          # kPrepTileH, kPrepTileW of csrc/image.hip


def _cfg(*overrides):
    from da_detect_amd.config import cfg

    c = cfg.clone()
    c.merge_from_list(list(overrides))
    return c


def _prepare(c, imgs, decisions, device, launches=None):
    """DeviceBatchPreparer on the images, and the same launch again into a NaN-filled buffer: whatever that one holds
    afterwards, the kernel wrote.  -> the ImageList over the NaN-filled buffer"""
    from da_detect_amd import _lib
    from da_detect_amd.data import device_prep as P
    from da_detect_amd.structures.image_list import ImageList

    prep = P.DeviceBatchPreparer(c, is_train=True)
    on_device = [torch.from_numpy(i).to(device) for i in imgs]
    calls = []
    real_call = _lib.call

    def counting_call(name, *args):
        calls.append(name)
        return real_call(name, *args)

    _lib.call = counting_call
    try:
        batch, _ = prep(on_device, None, decisions)
    finally:
        _lib.call = real_call
    if launches is not None:
        assert calls == ["dadet_image_prepare_batch"] * launches, calls
    again = torch.full(tuple(batch.tensors.shape), float("nan"), device=device).contiguous(memory_format=torch.channels_last)
    P.prepare_batch_into(on_device, decisions, c.INPUT.PIXEL_MEAN, c.INPUT.PIXEL_STD, c.INPUT.TO_BGR255, again)
    assert torch.equal(again, batch.tensors)
    return ImageList(again, batch.image_sizes)


def _check(c, batch, imgs, decisions):
    """every slot against the oracle's restatement of the host chain (itself pinned to Pillow), all padding zero"""
    from oracle.image_ref import preprocess

    got = batch.tensors.cpu().numpy()
    assert got.shape[0] == len(imgs) and batch.image_sizes == [d[0] for d in decisions]
    for i, (im, ((oh, ow), flip)) in enumerate(zip(imgs, decisions)):
        want = preprocess(im, oh, ow, flip, c.INPUT.PIXEL_MEAN, c.INPUT.PIXEL_STD, c.INPUT.TO_BGR255)
        assert np.array_equal(got[i, :, :oh, :ow], want), (i, im.shape, oh, ow, flip)
        pad = np.concatenate([got[i, :, oh:, :].ravel(), got[i, :, :oh, ow:].ravel()])
        assert np.array_equal(pad, np.zeros_like(pad)), (i, "padding")       # (NaN left behind fails this too)


def test_a_mixed_batch_in_one_launch(device):
    """A: the three images of test_device_batch_preparation_is_bit_exact — down-scale + flip, identity, mixed — one launch"""
    c = _cfg("DATALOADER.SIZE_DIVISIBILITY", 32)
    rng = np.random.default_rng(7)
    imgs = [_image(rng, 64, 128), _image(rng, 90, 100), _image(rng, 50, 120)]
    decisions = [((38, 75), True), ((90, 100), False), ((77, 50), True)]
    batch = _prepare(c, imgs, decisions, device, launches=1)
    assert tuple(batch.tensors.shape) == (3, 3, 96, 128)
    _check(c, batch, imgs, decisions)


def test_b_enlarging_odd_sizes_rgb_std(device):
    """B: 37x53 -> 61x131, both axes enlarged, widths no multiple of the tile or of 4, canvas = image, RGB with a std"""
    c = _cfg("DATALOADER.SIZE_DIVISIBILITY", 0, "INPUT.TO_BGR255", False, "INPUT.PIXEL_MEAN", [0.485, 0.456, 0.406],
             "INPUT.PIXEL_STD", [0.229, 0.224, 0.225])
    imgs = [_image(np.random.default_rng(11), 37, 53)]
    for flip in (False, True):
        decisions = [((61, 131), flip)]
        batch = _prepare(c, imgs, decisions, device, launches=1)
        assert tuple(batch.tensors.shape) == (1, 3, 61, 131)
        _check(c, batch, imgs, decisions)


def test_c_vertical_factor_beyond_one_chunk(device):
    """C: 256x40 -> 31x5 flipped: vertical factor 8.26 — one chunk of 64 input rows holds a 16-row tile up to factor 3, so
    the tiles here draw from about 150 rows and the accumulators carry over two chunk boundaries"""
    c = _cfg("DATALOADER.SIZE_DIVISIBILITY", 32)
    imgs = [_image(np.random.default_rng(12), 256, 40)]
    decisions = [((31, 5), True)]
    batch = _prepare(c, imgs, decisions, device, launches=1)
    _check(c, batch, imgs, decisions)
    want = np.asarray(Image.fromarray(imgs[0]).resize((5, 31), Image.BILINEAR))[:, ::-1].astype(np.float32)
    want = (want / np.float32(255.0))[:, :, ::-1] * np.float32(255.0) - np.asarray(c.INPUT.PIXEL_MEAN, np.float32)
    assert np.array_equal(batch.tensors[0, :, :31, :5].permute(1, 2, 0).cpu().numpy(), want.astype(np.float32))


@pytest.mark.parametrize("flip", [False, True])
def test_d_tile_edges(device, flip):
    """D: out_h in {T, T + 1} x out_w in {Tw, Tw + 1} for the 16 x 64 tile, in one batch of four"""
    c = _cfg("DATALOADER.SIZE_DIVISIBILITY", 32)
    rng = np.random.default_rng(13)
    imgs = [_image(rng, 23, 90) for _ in range(4)]
    decisions = [((oh, ow), flip) for oh in (TILE_H, TILE_H + 1) for ow in (TILE_W, TILE_W + 1)]
    batch = _prepare(c, imgs, decisions, device, launches=1)
    assert tuple(batch.tensors.shape) == (4, 3, 32, 96)
    _check(c, batch, imgs, decisions)


def test_e_eight_images_then_nine(device):
    """E: 8 random images in one launch; 9 take two (the wrapper sends chunks of 8)"""
    c = _cfg("DATALOADER.SIZE_DIVISIBILITY", 32)
    rng = np.random.default_rng(14)
    for n, launches in ((8, 1), (9, 2)):
        imgs = [_image(rng, int(rng.integers(16, 41)), int(rng.integers(16, 41))) for _ in range(n)]
        decisions = [((int(rng.integers(16, 41)), int(rng.integers(16, 41))), bool(rng.integers(0, 2))) for _ in range(n)]
        decisions[1] = ((imgs[1].shape[0], int(rng.integers(16, 41))), True)        # no vertical pass
        decisions[2] = ((int(rng.integers(16, 41)), imgs[2].shape[1]), True)        # no horizontal pass
        batch = _prepare(c, imgs, decisions, device, launches=launches)
        _check(c, batch, imgs, decisions)


def test_f_cityscapes_size_against_pillow(device):
    """F: 1024x2048 -> 600x1200 against Pillow directly"""
    c = _cfg("DATALOADER.SIZE_DIVISIBILITY", 32)
    img = _image(np.random.default_rng(1), 1024, 2048)
    batch = _prepare(c, [img], [((600, 1200), False)], device, launches=1)
    assert tuple(batch.tensors.shape) == (1, 3, 608, 1216)
    pil = np.asarray(Image.fromarray(img).resize((1200, 600), Image.BILINEAR)).astype(np.float32)
    want = (pil / np.float32(255.0))[:, :, ::-1] * np.float32(255.0) - np.asarray(c.INPUT.PIXEL_MEAN, np.float32)
    got = batch.tensors[0].permute(1, 2, 0).cpu().numpy()
    assert np.array_equal(got[:600, :1200], want.astype(np.float32))
    assert not got[600:].any() and not got[:, 1200:].any()


def test_bad_descriptors_are_refused(device):
    from da_detect_amd import _lib
    from da_detect_amd.data.device_prep import prepare_batch_into

    img = torch.zeros((20, 30, 3), dtype=torch.uint8, device=device)
    small = torch.empty((1, 3, 16, 32), dtype=torch.float32, device=device, memory_format=torch.channels_last)
    with pytest.raises(_lib.DadetError, match="does not fit"):
        prepare_batch_into([img], [((20, 30), False)], (0, 0, 0), (1, 1, 1), True, small)
    with pytest.raises(_lib.DadetError):
        prepare_batch_into([img.cpu()], [((20, 30), False)], (0, 0, 0), (1, 1, 1), True, small)


# ------------------------------------------------------------------------------------------------------ loaders
LOADER_SIZES = {"source": [(96, 192), (96, 160), (80, 192), (96, 192)], "target": [(90, 180), (96, 192), (96, 140), (64, 192)],
                "auxiliary": [(96, 192), (70, 150), (96, 192), (88, 192)]}


def _specs(tmp_path, names):
    rng = np.random.default_rng(0)
    return {k: _write_coco(str(tmp_path), k, 4, rng, sizes=LOADER_SIZES[k]) for k in names}


def _loader_cfg():
    return _cfg("SOLVER.IMS_PER_BATCH", 4, "SOLVER.MAX_ITER", 4, "DATALOADER.NUM_WORKERS", 0, "DATALOADER.SIZE_DIVISIBILITY", 32,
                "INPUT.MIN_SIZE_TRAIN", (96, 80), "INPUT.MAX_SIZE_TRAIN", 192, "MODEL.DOMAIN_ADAPTATION_ON", True)


def _same_field(got, want):
    from da_detect_amd.structures.image_list import ImageList

    if isinstance(want, ImageList):
        assert got.tensors.is_cuda
        assert torch.equal(got.tensors.cpu().contiguous(), want.tensors)           # layout may differ, values not
        assert [tuple(s) for s in got.image_sizes] == [tuple(s) for s in want.image_sizes]
    elif hasattr(want[0], "bbox"):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g.bbox.is_cuda and g.size == w.size and g.mode == w.mode and torch.equal(g.bbox.cpu(), w.bbox)
            assert sorted(g.fields()) == sorted(w.fields())
            for f in w.fields():
                assert torch.equal(g.get_field(f).cpu(), w.get_field(f)), f
    else:
        assert list(got) == list(want)


def test_da_loaders_equal_the_host_loaders(device, tmp_path):
    """make_da_data_loaders with and without device_prep, read the way do_da_train reads them (one batch of each per
    step): every batch collected first, compared afterwards — a staging or device buffer reused too early shows up"""
    from da_detect_amd.data.build import make_da_data_loaders

    specs = _specs(tmp_path, ("source", "target"))
    c = _loader_cfg()
    collected = {}
    for device_prep in (False, True):
        torch.manual_seed(9)
        random.seed(3)
        collected[device_prep] = list(zip(*make_da_data_loaders(c, specs, device_prep=device_prep)))
    torch.cuda.synchronize()
    assert len(collected[True]) == len(collected[False]) == 4
    flips = set()
    for got_step, want_step in zip(collected[True], collected[False]):
        for got, want in zip(got_step, want_step):              # per domain: (ImageList, targets, ids)
            assert len(got) == len(want) == 3
            for g, w in zip(got, want):
                _same_field(g, w)
            flips.add(tuple(want[0].tensors.shape[-2:]))
    assert len(flips) > 1                                        # the size draw mattered


def test_triplet_loader_equals_the_host_loader(device, tmp_path):
    from da_detect_amd.data.build import make_triplet_data_loader

    specs = _specs(tmp_path, ("source", "target", "auxiliary"))
    c = _loader_cfg()
    collected = {}
    for device_prep in (False, True):
        torch.manual_seed(9)
        random.seed(3)
        collected[device_prep] = list(make_triplet_data_loader(c, specs, device_prep=device_prep))
    torch.cuda.synchronize()
    assert len(collected[True]) == len(collected[False]) == 4
    for got, want in zip(collected[True], collected[False]):
        assert len(got) == len(want) == 9
        for g, w in zip(got, want):
            _same_field(g, w)


# ---------------------------------------------------------------------------------------- test-time augmentation
def _same_detections(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.size == y.size and torch.equal(x.bbox, y.bbox)
        assert torch.equal(x.get_field("labels"), y.get_field("labels"))
        assert torch.equal(x.get_field("scores"), y.get_field("scores"))


def test_augmentation_from_uint8_tensors_equals_the_pil_path(device):
    """H_FLIP and one scale with SCALE_H_FLIP: four passes; the stand-in detector's detections — and what it was given in
    every pass (sizes, sums over the valid region, probe pixels) — are the same from uint8 tensors as from PIL images,
    and the tensor path resizes nothing on the host"""
    from da_detect_amd.data import transforms as T
    from da_detect_amd.engine.bbox_aug import im_detect_bbox_aug
    from da_detect_amd.structures.bounding_box import BoxList

    c = _cfg("TEST.BBOX_AUG.ENABLED", True, "TEST.BBOX_AUG.H_FLIP", True, "TEST.BBOX_AUG.SCALES", (48,),
             "TEST.BBOX_AUG.MAX_SIZE", 96, "TEST.BBOX_AUG.SCALE_H_FLIP", True, "INPUT.MIN_SIZE_TEST", 60,
             "INPUT.MAX_SIZE_TEST", 110, "MODEL.ROI_BOX_HEAD.NUM_CLASSES", 4, "DATALOADER.SIZE_DIVISIBILITY", 32)
    pixels = make_images()
    runs = {}
    for kind in ("pil", "raw"):
        model = StubDetector(lambda boxes, size: BoxList(boxes, size, mode="xyxy"), num_classes=4)
        model.cfg = c
        images = [Image.fromarray(p) for p in pixels] if kind == "pil" else [torch.from_numpy(p) for p in pixels]
        host_resize = T.Resize.__call__
        if kind == "raw":
            def refuse(self, image, target):
                raise AssertionError("the tensor path must not resize on the host")
            T.Resize.__call__ = refuse
        try:
            with torch.no_grad():
                runs[kind] = (im_detect_bbox_aug(model, images, device), model.calls)
        finally:
            T.Resize.__call__ = host_resize
    assert len(runs["pil"][1]) == len(runs["raw"][1]) == 4
    for raw_call, pil_call in zip(runs["raw"][1], runs["pil"][1]):
        for key in ("padded", "sizes", "probes", "left_brighter"):
            assert raw_call[key] == pil_call[key], key
        # (a sum over all pixels in float64: the two batches differ in memory layout, so in the order of the additions)
        np.testing.assert_allclose(raw_call["sums"], pil_call["sums"], rtol=1e-12)
    assert sum(len(d) for d in runs["pil"][0]) > 0
    _same_detections(runs["raw"][0], runs["pil"][0])


def test_augmentation_loader_uploads_each_image_once(device, tmp_path):
    """make_test_data_loader(device_prep=True) under TEST.BBOX_AUG.ENABLED: uint8 device tensors, unbatched"""
    from da_detect_amd.data.build import make_test_data_loader
    from da_detect_amd.data.datasets import COCODataset
    from da_detect_amd.data.transforms import build_transforms

    ann, root = _specs(tmp_path, ("target",))["target"]
    c = _cfg("TEST.BBOX_AUG.ENABLED", True, "TEST.IMS_PER_BATCH", 2, "DATALOADER.NUM_WORKERS", 0)
    ds = COCODataset(ann, root, remove_images_without_annotations=False, transforms=build_transforms(c, False))
    batches = list(make_test_data_loader(c, ds, device_prep=True))
    torch.cuda.synchronize()
    assert [list(b[2]) for b in batches] == [[0, 1], [2, 3]]
    for images, _, ids in batches:
        for im, i in zip(images, ids):
            want = np.array(Image.open(os.path.join(root, "im%d.png" % i)).convert("RGB"))
            assert im.is_cuda and im.dtype == torch.uint8 and np.array_equal(im.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------- end to end
def _iteration_zero(log):
    line = [ln for ln in log.splitlines() if "iter: 0 " in ln]
    assert len(line) == 1, log[-2000:]
    return re.findall(r"(\S*loss\S*): (\S+) \(", line[0])


def test_training_entry_point_with_device_prep(tmp_path):
    """tools/train_net_da.py --device-prep on the tiny dataset of test_training_entry_point_on_a_tiny_dataset: status 0, and
    the logged losses of iteration 0 are those of the run without the flag (same seed, same batches)"""
    rng = np.random.default_rng(0)
    specs = {"source": _write_coco(str(tmp_path), "source", 4, rng, sizes=[(96, 192), (96, 160), (80, 192), (96, 192)]),
             "target": _write_coco(str(tmp_path), "target", 4, rng, sizes=[(90, 180), (96, 192), (96, 140), (64, 192)])}
    logs = {}
    for flag in ((), ("--device-prep",)):
        out = str(tmp_path / ("out%d" % len(flag)))
        os.makedirs(out)
        cmd = [sys.executable, os.path.join(ROOT, "tools", "train_net_da.py"), "--config-file",
               os.path.join(ROOT, "configs/da_faster_rcnn/e2e_da_faster_rcnn_R_50_C4_cityscapes_to_foggy_cityscapes.yaml"),
               "--source", ",".join(specs["source"]), "--target", ",".join(specs["target"])] + list(flag) + [
               "SOLVER.MAX_ITER", "4", "SOLVER.CHECKPOINT_PERIOD", "0", "DATALOADER.NUM_WORKERS", "0",
               "INPUT.MIN_SIZE_TRAIN", "(96,)", "INPUT.MAX_SIZE_TRAIN", "192", "MODEL.OUTPUT_DIR", out, "MODEL.WEIGHT", ""]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stderr[-2000:]
        assert os.path.exists(os.path.join(out, "model_final.pth"))
        logs[flag] = res.stderr
    with_flag, without = _iteration_zero(logs[("--device-prep",)]), _iteration_zero(logs[()])
    print(with_flag, without)
    assert len(without) >= 5 and with_flag == without


@pytest.mark.parametrize("aug", [False, True])
def test_evaluation_loop_with_device_prep(device, tmp_path, aug):
    """engine.inference over make_test_data_loader with and without device_prep — plain batches, and the augmentation
    passes (H_FLIP + one scale) selected by the raw collator — on the seeded da_plain evaluation model: the same records"""
    import json

    from da_detect_amd.data.build import make_test_data_loader
    from da_detect_amd.data.datasets import COCODataset
    from da_detect_amd.data.transforms import build_transforms
    from da_detect_amd.engine.inference import inference
    from test_bbox_aug import _eval_model

    ann, root = _write_coco(str(tmp_path), "val", 3, np.random.default_rng(6), sizes=[(96, 160), (90, 150), (96, 128)])
    data = json.load(open(ann))
    data["categories"] = [{"id": 24 + k, "name": "c%d" % k} for k in range(8)]      # the model's eight classes
    json.dump(data, open(ann, "w"))
    overrides = ["MODEL.ROI_HEADS.SCORE_THRESH", 0.02, "TEST.IMS_PER_BATCH", 2, "DATALOADER.NUM_WORKERS", 0]
    if aug:
        overrides += ["TEST.BBOX_AUG.ENABLED", True, "TEST.BBOX_AUG.H_FLIP", True, "TEST.BBOX_AUG.SCALES", (160,)]
    c, model, _, _ = _eval_model(device, *overrides)
    records = {}
    for device_prep in (False, True):
        ds = COCODataset(ann, root, remove_images_without_annotations=False, transforms=build_transforms(c, False))
        loader = make_test_data_loader(c, ds, device_prep=device_prep)
        with torch.no_grad():
            records[device_prep] = inference(model, loader, "val", device=device)
    assert len(records[False]) > 0 and records[True] == records[False]


def test_scoring_entry_point_with_device_prep(tmp_path):
    """tools/score_net_da.py --config-file ... --device-prep with test-time augmentation: the evaluation pass runs in the
    tool's own process on the device input pipeline, leaves one prediction per image and the table is scored from them"""
    import json

    ann, root = _write_coco(str(tmp_path), "val", 3, np.random.default_rng(8), sizes=[(96, 192), (80, 160), (96, 128)])
    out = str(tmp_path / "out")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "score_net_da.py"), "--dataset", "%s,%s" % (ann, root), "--config-file",
           os.path.join(ROOT, "configs/da_faster_rcnn/e2e_da_faster_rcnn_R_50_C4_cityscapes_to_foggy_cityscapes.yaml"),
           "--output-dir", out, "--device-prep", "DATALOADER.NUM_WORKERS", "0", "INPUT.MIN_SIZE_TEST", "96",
           "INPUT.MAX_SIZE_TEST", "192", "MODEL.WEIGHT", "", "MODEL.ROI_BOX_HEAD.NUM_CLASSES", "3", "TEST.IMS_PER_BATCH", "2",
           "MODEL.ROI_HEADS.SCORE_THRESH", "0.0", "TEST.BBOX_AUG.ENABLED", "True", "TEST.BBOX_AUG.H_FLIP", "True"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    folder = os.path.join(out, "inference", "val")
    predictions = torch.load(os.path.join(folder, "predictions.pth"), weights_only=False)
    assert len(predictions) == 3 and [p.size for p in predictions] == [(192, 96), (192, 96), (128, 96)]
    records = json.load(open(os.path.join(folder, "bbox.json")))
    assert len(records) > 0 and {r["image_id"] for r in records} <= {100, 101, 102}
    assert "COCO box AP" in res.stderr
