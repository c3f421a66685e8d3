"""Host side of the device input pipeline (data/datasets.py RawImage, the Raw* collators, data/build.py device_prep=,
data/device_prep.py DevicePrepLoader, the dadet_image_prepare_batch binding): what can be pinned without a GPU.  The
pixels themselves are pinned in tests/test_device_input_gpu.py."""
import ctypes
import inspect
import os
import random
import re

import numpy as np
import pytest
import torch

from test_data_pipeline import _write_coco
from test_voc_eval import TWO_IMAGES, write_voc_tree

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
pytest.importorskip("PIL")
from PIL import Image  # noqa: E402

SIZES = [(96, 192), (96, 160), (80, 192), (90, 140)]


def _cfg(*overrides):
    from da_detect_amd.config import cfg

    c = cfg.clone()
    c.merge_from_list(["SOLVER.IMS_PER_BATCH", 4, "SOLVER.MAX_ITER", 3, "DATALOADER.NUM_WORKERS", 0,
                       "DATALOADER.SIZE_DIVISIBILITY", 32, "INPUT.MIN_SIZE_TRAIN", (96, 80), "INPUT.MAX_SIZE_TRAIN", 192,
                       "MODEL.DOMAIN_ADAPTATION_ON", True] + list(overrides))
    return c


def _same_boxes(a, b):
    assert a.size == b.size and a.mode == b.mode and torch.equal(a.bbox, b.bbox)
    assert sorted(a.fields()) == sorted(b.fields())
    for f in a.fields():
        assert torch.equal(a.get_field(f), b.get_field(f)), f


def _check_sample(host_img, host_tgt, raw_img, raw_tgt, plain_tgt, pixels):
    """the decisions a raw sample carries are the ones the host chain applied under the same seed — read off the host
    sample's size, its pixels (oracle restatement of the chain under those decisions) and its transformed target"""
    from da_detect_amd.config import cfg
    from da_detect_amd.data.datasets import RawImage
    from oracle.image_ref import preprocess

    assert isinstance(raw_img, RawImage) and raw_img.pixels.dtype == torch.uint8 and not raw_img.pixels.is_cuda
    assert np.array_equal(raw_img.pixels.numpy(), pixels)
    (oh, ow), flip = raw_img.decision
    assert tuple(host_img.shape) == (3, oh, ow)
    want = preprocess(pixels, oh, ow, flip, cfg.INPUT.PIXEL_MEAN, cfg.INPUT.PIXEL_STD, cfg.INPUT.TO_BGR255)
    assert np.array_equal(host_img.numpy(), want)
    _same_boxes(raw_tgt, plain_tgt)                       # untransformed: the host path's target before its transforms
    moved = plain_tgt.resize((ow, oh))
    _same_boxes(host_tgt, moved.transpose(0) if flip else moved)
    return (oh, ow), flip


def test_raw_samples_carry_the_decisions_of_the_host_chain(tmp_path):
    from da_detect_amd.data.datasets import COCODataset
    from da_detect_amd.data.transforms import build_transforms

    ann, root = _write_coco(str(tmp_path), "source", 4, np.random.default_rng(0), sizes=SIZES)
    tf = build_transforms(_cfg(), True)
    host = COCODataset(ann, root, True, transforms=tf)
    raw = COCODataset(ann, root, True, transforms=tf, decode_to_tensor=True)
    plain = COCODataset(ann, root, True, transforms=None)
    assert len(host) == len(raw) == 3
    seen = set()
    for seed in range(6):
        for i in range(len(host)):
            random.seed(seed * 10 + i)
            h_img, h_tgt, h_idx = host[i]
            after_host = random.random()
            random.seed(seed * 10 + i)
            r_img, r_tgt, r_idx = raw[i]
            assert random.random() == after_host and h_idx == r_idx == i      # the same number of draws
            pixels = np.array(Image.open(os.path.join(root, host.get_img_info(i)["file_name"])).convert("RGB"))
            (oh, ow), flip = _check_sample(h_img, h_tgt, r_img, r_tgt, plain[i][1], pixels)
            seen.add((min(oh, ow), flip))
    assert seen == {(96, True), (96, False), (80, True), (80, False)}     # the size draw and the toss both mattered
    # without transforms the sample stays as it was: pixels only
    bare = COCODataset(ann, root, True, decode_to_tensor=True)[0][0]
    assert isinstance(bare, torch.Tensor) and bare.dtype == torch.uint8 and tuple(bare.shape) == (96, 192, 3)


def test_triplet_and_voc_datasets_follow_suit(tmp_path):
    from da_detect_amd.data.datasets import COCODataset, PascalVOCDataset, RawImage, TripletDataset
    from da_detect_amd.data.transforms import build_transforms

    rng = np.random.default_rng(1)
    specs = [_write_coco(str(tmp_path), k, 4, rng, sizes=SIZES) for k in ("source", "target", "auxiliary")]
    tf = build_transforms(_cfg(), True)
    host = TripletDataset([COCODataset(a, r, True, transforms=tf, is_source=k == 0) for k, (a, r) in enumerate(specs)])
    raw = TripletDataset([COCODataset(a, r, True, transforms=tf, is_source=k == 0, decode_to_tensor=True)
                          for k, (a, r) in enumerate(specs)])
    for i in range(len(host)):
        random.seed(40 + i)
        h = host[i]
        random.seed(40 + i)
        r = raw[i]
        assert len(r) == len(h) == 9 and r[6:] == h[6:]
        for k in (0, 2, 4):                                # source, then target, then auxiliary: three (size, toss) pairs
            assert isinstance(r[k], RawImage) and tuple(h[k].shape[-2:]) == r[k].decision[0]
        # the target / auxiliary annotations are copies of the source sample's with their own domain flag, in both
        (oh, ow), flip = r[0].decision
        moved = r[1].resize((ow, oh))
        _same_boxes(h[1], moved.transpose(0) if flip else moved)
        assert torch.equal(r[3].bbox, r[1].bbox) and not r[3].get_field("is_source").any()
        assert torch.equal(h[3].bbox, h[1].bbox) and torch.equal(h[5].bbox, h[1].bbox)

    voc_root = write_voc_tree(tmp_path / "voc", TWO_IMAGES)
    v_host = PascalVOCDataset(voc_root, "test", transforms=tf)
    v_raw = PascalVOCDataset(voc_root, "test", transforms=tf, decode_to_tensor=True)
    for i in range(2):
        random.seed(7 + i)
        h_img, h_tgt, _ = v_host[i]
        random.seed(7 + i)
        r_img, r_tgt, _ = v_raw[i]
        (oh, ow), flip = r_img.decision
        assert tuple(h_img.shape) == (3, oh, ow) and tuple(r_img.pixels.shape) == (TWO_IMAGES[i][2], TWO_IMAGES[i][1], 3)
        moved = r_tgt.resize((ow, oh))
        _same_boxes(h_tgt, moved.transpose(0) if flip else moved)
    assert isinstance(PascalVOCDataset(voc_root, "test", decode_to_tensor=True)[0][0], torch.Tensor)


def test_raw_collators_keep_field_order_and_arity():
    from da_detect_amd.data.collate_batch import BBoxAugCollator, RawBatchCollator_triplet, RawBBoxAugCollator

    samples = [tuple("%s%d" % (f, i) for f in ("is", "ts", "ip", "tp", "in", "tn", "a", "b", "c")) for i in range(2)]
    out = RawBatchCollator_triplet()(samples)
    assert len(out) == 9
    assert [list(f) for f in out] == [["%s%d" % (f, i) for i in range(2)]
                                      for f in ("is", "ts", "ip", "tp", "in", "tn", "a", "b", "c")]
    assert all(isinstance(out[k], list) for k in (0, 2, 4))
    tta = RawBBoxAugCollator()
    assert isinstance(tta, BBoxAugCollator)                  # engine.inference selects the augmentation passes by this
    images, targets, ids = tta([("i0", "t0", 0), ("i1", "t1", 1)])
    assert (images, targets, ids) == (("i0", "i1"), ("t0", "t1"), (0, 1))
    assert tta([("i0", "t0", 0), ("i1", "t1", 1)]) == BBoxAugCollator()([("i0", "t0", 0), ("i1", "t1", 1)])


def _first_batches(loaders):
    return [next(iter(loader)) for loader in loaders]


def test_loader_surface_and_defaults(tmp_path):
    from da_detect_amd.data import build as B
    from da_detect_amd.data.collate_batch import (BatchCollator, BatchCollator_triplet, RawBatchCollator,
                                                  RawBatchCollator_triplet, RawBBoxAugCollator)
    from da_detect_amd.data.datasets import COCODataset
    from da_detect_amd.data.device_prep import DevicePrepLoader
    from da_detect_amd.data.transforms import build_transforms
    from da_detect_amd.structures.image_list import to_image_list

    rng = np.random.default_rng(2)
    specs = {k: _write_coco(str(tmp_path), k, 4, rng, sizes=SIZES) for k in ("source", "target", "auxiliary")}
    c = _cfg()
    for name in ("make_da_data_loaders", "make_triplet_data_loader", "make_test_data_loader"):
        assert inspect.signature(getattr(B, name)).parameters["device_prep"].default is False
    for name in ("make_data_loader", "make_data_loader_da"):       # the reference's signatures are not touched
        assert list(inspect.signature(getattr(B, name)).parameters) == (
            ["cfg", "is_train", "is_source", "is_negative", "is_distributed", "is_for_period", "start_iter"]
            if name == "make_data_loader" else
            ["cfg", "is_source", "is_train", "is_negative", "is_distributed", "is_for_period", "start_iter"])

    # defaults: today's loaders and today's first batch (the host chain restated here from its parts)
    random.seed(3)
    loaders = B.make_da_data_loaders(c, {k: specs[k] for k in ("source", "target")})
    assert all(type(l) is torch.utils.data.DataLoader and type(l.collate_fn) is BatchCollator for l in loaders)
    random.seed(3)
    got = next(iter(loaders[0]))
    ds = COCODataset(*specs["source"], remove_images_without_annotations=True, transforms=build_transforms(c, True))
    order = list(got[2])                                      # the sampler's shuffle; the transforms draw from `random`
    random.seed(3)
    samples = [ds[i] for i in order]
    want = to_image_list([s[0] for s in samples], 32)
    assert len(order) == 2 and torch.equal(got[0].tensors, want.tensors) and list(got[2]) == list(order)
    assert [tuple(s) for s in got[0].image_sizes] == [tuple(s[0].shape[-2:]) for s in samples]
    for t, s in zip(got[1], samples):
        _same_boxes(t, s[1])
    trip = B.make_triplet_data_loader(c, specs)
    assert type(trip) is torch.utils.data.DataLoader and type(trip.collate_fn) is BatchCollator_triplet
    assert len(next(iter(trip))) == 9

    # device_prep=True: the wrapper with the surface inference / do_da_train read, built without touching a device
    raw = B.make_da_data_loaders(c, {k: specs[k] for k in ("source", "target")}, device_prep=True)
    for wrapped, plain in zip(raw, loaders):
        assert isinstance(wrapped, DevicePrepLoader) and isinstance(wrapped.collate_fn, RawBatchCollator)
        assert len(wrapped) == len(plain) == 3 and len(wrapped.dataset) == len(plain.dataset)
        assert wrapped.dataset.decode_to_tensor and wrapped.batch_sampler is wrapped.loader.batch_sampler
        assert [len(b) for b in wrapped.batch_sampler] == [len(b) for b in plain.batch_sampler]
    rtrip = B.make_triplet_data_loader(c, specs, device_prep=True)
    assert isinstance(rtrip, DevicePrepLoader) and isinstance(rtrip.collate_fn, RawBatchCollator_triplet) and len(rtrip) == 3
    for aug, kind in ((False, RawBatchCollator), (True, RawBBoxAugCollator)):
        ct = _cfg("TEST.BBOX_AUG.ENABLED", aug, "TEST.IMS_PER_BATCH", 2)
        ds = COCODataset(*specs["target"], remove_images_without_annotations=False, transforms=build_transforms(ct, False))
        test_loader = B.make_test_data_loader(ct, ds, device_prep=True)
        assert isinstance(test_loader, DevicePrepLoader) and type(test_loader.collate_fn) is kind
        assert test_loader.dataset is ds and ds.decode_to_tensor and len(test_loader) == 2
        first = next(iter(test_loader.loader))               # the raw loader underneath: CPU tensors only
        assert all(not (im.pixels if hasattr(im, "pixels") else im).is_cuda for im in first[0])
        assert all(hasattr(im, "decision") != aug for im in first[0])


def test_workers_deliver_cpu_tensors(tmp_path):
    """two worker processes: samples arrive as CPU tensors with their decisions, the same as without workers"""
    from da_detect_amd.data import build as B

    rng = np.random.default_rng(4)
    specs = {k: _write_coco(str(tmp_path), k, 4, rng, sizes=SIZES) for k in ("source", "target")}
    c = _cfg("DATALOADER.NUM_WORKERS", 2)
    raw = B.make_da_data_loaders(c, specs, device_prep=True)[0].loader
    for images, targets, ids in raw:
        assert all(im.pixels.dtype == torch.uint8 and not im.pixels.is_cuda and len(im.decision) == 2 for im in images)
        assert all(not t.bbox.is_cuda for t in targets)


def test_prepare_batch_abi():
    from da_detect_amd import _lib

    header = open(os.path.join(ROOT, "include", "dadet.h")).read()
    proto = re.search(r"\bint\s+dadet_image_prepare_batch\s*\(([^;]*)\)\s*;", header)
    assert proto, "include/dadet.h does not declare dadet_image_prepare_batch"
    assert len(proto.group(1).split(",")) == len(_lib._SIGNATURES["dadet_image_prepare_batch"]) == 10
    assert "dadet_image_prepare_batch" in _lib.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "dadet_image_prepare_batch")
    # the descriptor mirrors the header's struct field for field: five pointers, eight ints, 8 per launch
    body = re.search(r"typedef struct dadet_image_item \{(.*?)\} dadet_image_item;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip()
             for n in re.sub(r"^\s*(const\s+void\s*\*|int)", "", decl.strip()).split(",")]
    assert names == [n for n, _ in _lib.ImageItem._fields_]
    assert ctypes.sizeof(_lib.ImageItem) == 5 * 8 + 8 * 4
    assert int(re.search(r"#define DADET_IMAGE_BATCH_MAX (\d+)", header).group(1)) == _lib.IMAGE_BATCH_MAX == 8
