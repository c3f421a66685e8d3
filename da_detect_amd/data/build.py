"""Data-loader assembly (reference: maskrcnn_benchmark/data/build.py:67-419): dataset construction from the path
catalog, aspect-ratio grouping, the distributed / grouped / iteration-based sampler stack, and the source / target /
auxiliary pairing of the DA trainers.

Two entry families over the same machinery:
  * the reference's own — `make_data_loader(cfg, is_train, is_source, is_negative, is_distributed, is_for_period,
    start_iter)` and `make_data_loader_da(cfg, is_source=[...], ...)` — dataset NAMES from cfg.DATASETS resolved through
    `DatasetCatalog` of the file cfg.PATHS_CATALOG (what tools/train_net_triplet.py:108-170 calls);
  * explicit (annotation file, image root) pairs — `make_da_data_loaders`, `make_triplet_data_loader`
    (tools/train_net_da.py).
"""
import bisect
import logging

import torch

from ..utils.comm import get_world_size
from ..utils.imports import load_paths_catalog
from . import datasets as D
from . import samplers
from .collate_batch import (BatchCollator, BatchCollator_triplet, BBoxAugCollator, RawBatchCollator, RawBatchCollator_triplet,
                            RawBBoxAugCollator)
from .datasets import COCODataset, TripletDataset
from .transforms import build_transforms


def _quantize(x, bins):
    bins = sorted(bins)
    return [bisect.bisect_right(bins, v) for v in x]


def _compute_aspect_ratios(dataset):
    out = []
    for i in range(len(dataset)):
        info = dataset.get_img_info(i)
        out.append(float(info["height"]) / float(info["width"]))
    return out


def make_data_sampler(dataset, shuffle, distributed):
    if distributed:
        return samplers.DistributedSampler(dataset, shuffle=shuffle)
    if shuffle:
        return torch.utils.data.sampler.RandomSampler(dataset)
    return torch.utils.data.sampler.SequentialSampler(dataset)


def make_batch_data_sampler(dataset, sampler, aspect_grouping, images_per_batch, num_iters=None, start_iter=0):
    """build.py:176-196"""
    if aspect_grouping:
        if not isinstance(aspect_grouping, (list, tuple)):
            aspect_grouping = [aspect_grouping]
        group_ids = _quantize(_compute_aspect_ratios(dataset), aspect_grouping)
        batch_sampler = samplers.GroupedBatchSampler(sampler, group_ids, images_per_batch, drop_uneven=False)
    else:
        batch_sampler = torch.utils.data.sampler.BatchSampler(sampler, images_per_batch, drop_last=False)
    if num_iters is not None:
        batch_sampler = samplers.IterationBasedBatchSampler(batch_sampler, num_iters, start_iter)
    return batch_sampler


def images_per_gpu(cfg, is_train, domain_share=1):
    """build.py:232-246: IMS_PER_BATCH // num_gpus, and with DOMAIN_ADAPTATION_ON every loader (source, target,
    auxiliary, or the triplet loader) takes IMS_PER_BATCH // (2 * num_gpus) samples per step (`domain_share` = 2)"""
    total = cfg.SOLVER.IMS_PER_BATCH if is_train else cfg.TEST.IMS_PER_BATCH
    world = get_world_size()
    assert total % (world * domain_share) == 0, \
        "IMS_PER_BATCH ({}) must be divisible by the number of GPUs ({}) x domains ({})".format(total, world, domain_share)
    return total // (world * domain_share)


def _loader_for(cfg, dataset, per_gpu, shuffle, is_distributed, num_iters, start_iter, collator):
    sampler = make_data_sampler(dataset, shuffle, is_distributed)
    batch_sampler = make_batch_data_sampler(dataset, sampler, [1] if cfg.DATALOADER.ASPECT_RATIO_GROUPING else [],
                                            per_gpu, num_iters, start_iter)
    return torch.utils.data.DataLoader(dataset, num_workers=cfg.DATALOADER.NUM_WORKERS, batch_sampler=batch_sampler,
                                       collate_fn=collator)


# ------------------------------------------------------------------------------------ the reference's entry points
def _catalog(cfg):
    return load_paths_catalog(cfg.PATHS_CATALOG).DatasetCatalog


def _from_catalog(name, catalog, transforms, is_train, is_source):
    """one dataset from its catalog entry (build.py:84-103, 141-169)"""
    data = catalog.get(name)
    if data["factory"] == "CityscapesDataset":
        from .cityscapes import CityscapesDataset as factory
    else:
        factory = getattr(D, data["factory"])
    args = dict(data["args"])
    if data["factory"] in ("COCODataset", "CityscapesDataset"):
        args["remove_images_without_annotations"] = is_train
    if data["factory"] == "PascalVOCDataset":
        args["use_difficult"] = not is_train
    args["transforms"] = transforms
    args["is_source"] = is_source
    return factory(**args)


def build_dataset(dataset_list, transforms, dataset_catalog, is_train=True, is_source=True):
    """training: ONE (possibly concatenated) dataset in a list; testing: one per name (build.py:124-181)"""
    if not isinstance(dataset_list, (list, tuple)):
        raise RuntimeError("dataset_list should be a list of strings, got {}".format(dataset_list))
    datasets = [_from_catalog(n, dataset_catalog, transforms, is_train, is_source) for n in dataset_list]
    if not is_train:
        return datasets
    return [datasets[0] if len(datasets) == 1 else D.ConcatDataset(datasets)]


def build_dataset_da(dataset_list, transforms, dataset_catalog, is_source, is_train=True):
    """`is_source` is a list parallel to `dataset_list` = [source, target, auxiliary]; training: the index-aligned
    triplet dataset in a list, testing: the three datasets (build.py:67-121)"""
    if not isinstance(dataset_list, (list, tuple)):
        raise RuntimeError("dataset_list should be a list of strings, got {}".format(dataset_list))
    datasets = [_from_catalog(n, dataset_catalog, transforms, is_train, src)
                for n, src in zip(dataset_list, is_source)]
    if not is_train:
        return datasets
    return [TripletDataset(datasets)]


def _batch_plan(cfg, is_train, is_distributed, start_iter):
    """-> (images per GPU and loader, shuffle, number of iterations, start_iter) — build.py:233-258"""
    if is_train:
        per_gpu = images_per_gpu(cfg, True, 2 if cfg.MODEL.DOMAIN_ADAPTATION_ON else 1)
        plan = per_gpu, True, cfg.SOLVER.MAX_ITER, start_iter
    else:
        plan = images_per_gpu(cfg, False), bool(is_distributed), None, 0
    if plan[0] > 1:
        logging.getLogger(__name__).warning(
            "More than one image per GPU and loader: memory grows with it; reduce SOLVER.IMS_PER_BATCH / "
            "TEST.IMS_PER_BATCH if needed (and rescale the learning rate and schedule for training).")
    return plan


def make_data_loader(cfg, is_train=True, is_source=True, is_negative=False, is_distributed=False, is_for_period=False,
                     start_iter=0):
    """reference signature (build.py:232-329).  Training: the loader of ONE domain — SOURCE_TRAIN, TARGET_TRAIN or
    TARGET_TRAIN_negative under DOMAIN_ADAPTATION_ON (each IMS_PER_BATCH // (2 * GPUs) images per step), TRAIN
    otherwise; testing: a list with one loader per cfg.DATASETS.TEST entry."""
    per_gpu, shuffle, num_iters, start_iter = _batch_plan(cfg, is_train, is_distributed, start_iter)
    if not is_train:
        names = cfg.DATASETS.TEST
    elif not cfg.MODEL.DOMAIN_ADAPTATION_ON:
        names = cfg.DATASETS.TRAIN
    elif is_source:
        names = cfg.DATASETS.SOURCE_TRAIN
    else:
        names = cfg.DATASETS.TARGET_TRAIN_negative if is_negative else cfg.DATASETS.TARGET_TRAIN
    # evaluation with test-time augmentation: untransformed images, unbatched (build.py:155,168)
    aug = (not is_train) and cfg.TEST.BBOX_AUG.ENABLED
    transforms = None if aug else build_transforms(cfg, is_train)
    collator = BBoxAugCollator() if aug else BatchCollator(cfg.DATALOADER.SIZE_DIVISIBILITY)
    datasets = build_dataset(list(names), transforms, _catalog(cfg), is_train, is_source)
    loaders = [_loader_for(cfg, ds, per_gpu, shuffle, is_distributed, num_iters, start_iter, collator) for ds in datasets]
    if is_train:
        assert len(loaders) == 1
        return loaders[0]
    return loaders


def make_data_loader_da(cfg, is_source, is_train=True, is_negative=False, is_distributed=False, is_for_period=False,
                        start_iter=0):
    """reference signature (build.py:332-419): the ALIGNED triplet loader over (SOURCE_TRAIN[0], TARGET_TRAIN[0],
    TARGET_TRAIN_negative[0]); `is_source` = [True, False, False] flags the three domains.  Every batch is the nine
    fields of BatchCollator_triplet."""
    per_gpu, shuffle, num_iters, start_iter = _batch_plan(cfg, is_train, is_distributed, start_iter)
    if is_train:
        names = [cfg.DATASETS.SOURCE_TRAIN[0], cfg.DATASETS.TARGET_TRAIN[0], cfg.DATASETS.TARGET_TRAIN_negative[0]]
    else:
        names = list(cfg.DATASETS.TEST)
    single = is_train or is_for_period
    datasets = build_dataset_da(names, build_transforms(cfg, is_train), _catalog(cfg), is_source, single)
    loaders = [_loader_for(cfg, ds, per_gpu, shuffle, is_distributed, num_iters, start_iter,
                           BatchCollator_triplet(cfg.DATALOADER.SIZE_DIVISIBILITY)) for ds in datasets]
    if single:
        assert len(loaders) == 1
        return loaders[0]
    return loaders


# ------------------------------------------------------------------------- explicit (annotation file, image root) pairs
def _train_loader(cfg, dataset, is_distributed, start_iter, collator):
    return _loader_for(cfg, dataset, images_per_gpu(cfg, True, 2), True, is_distributed, cfg.SOLVER.MAX_ITER,
                       start_iter, collator)


def _decode_to_tensor(dataset):
    """switch an already constructed dataset (or every part of a concatenation / triplet) to raw samples"""
    parts = getattr(dataset, "datasets", None) or [getattr(dataset, n) for n in ("dataset_s", "dataset_p", "dataset_n")
                                                    if hasattr(dataset, n)]
    for part in parts:
        _decode_to_tensor(part)
    if not parts:
        dataset.decode_to_tensor = True


def _device_prep_loader(cfg, loader, is_train):
    from .device_prep import DeviceBatchPreparer, DevicePrepLoader

    return DevicePrepLoader(loader, DeviceBatchPreparer(cfg, is_train))


def make_test_data_loader(cfg, dataset, is_distributed=False, device_prep=False):
    """evaluation loader over an already constructed dataset (sequential, or sharded by rank when distributed).  With
    cfg.TEST.BBOX_AUG.ENABLED the samples leave it untransformed and unbatched (transforms=None and BBoxAugCollator,
    build.py:155,168): the dataset's transforms are taken off here, the augmentation passes apply their own.
    `device_prep=True`: the dataset hands out decoded pixels (with the decisions of its transforms) and the batches are
    prepared on the device (data/device_prep.py DevicePrepLoader); under test-time augmentation each image is uploaded
    once and the passes prepare their inputs from it."""
    collator = RawBatchCollator() if device_prep else BatchCollator(cfg.DATALOADER.SIZE_DIVISIBILITY)
    if cfg.TEST.BBOX_AUG.ENABLED:
        dataset._transforms = None
        collator = RawBBoxAugCollator() if device_prep else BBoxAugCollator()
    if device_prep:
        _decode_to_tensor(dataset)
    loader = _loader_for(cfg, dataset, images_per_gpu(cfg, False), bool(is_distributed), is_distributed, None, 0, collator)
    return _device_prep_loader(cfg, loader, False) if device_prep else loader


RAIN_PREFIX = "rain:"
CITYSCAPES_PREFIX = "cityscapes:"


def parse_dataset_spec(text):
    """a tool's dataset argument -> the (first, second) pair `dataset_from_spec` takes: `ann.json,imgdir`, `voc:DIR,SPLIT`,
    `rain:MASKDIR` (second = "") or `cityscapes:ROOT,SPLIT[,foggy[=BETA]|rain][,caronly]` (second keeps the options)"""
    if text.startswith(RAIN_PREFIX):
        return text, ""
    if text.startswith(CITYSCAPES_PREFIX):
        first, second = text.split(",", 1)
        from .cityscapes import parse_options

        parse_options(second)
        return first, second
    first, second = text.split(",")
    return first, second


def is_rain_spec(spec):
    return spec[0].startswith(RAIN_PREFIX)


def dataset_from_spec(spec, transforms=None, is_train=True, is_source=True, decode_to_tensor=False, source_spec=None,
                      device=None):
    """spec = (ann_file, image_root) for a COCO-style dataset, or ("voc:" + data_dir, split) for one in PASCAL VOC layout
    (the command-line form `voc:DIR,SPLIT` of the tools); the train / test switches are those of `_from_catalog`.
    ("rain:" + mask_dir, "") — the tools' `rain:MASKDIR` — is the rainy rendering of `source_spec`'s images, synthesised per
    sample from the rain masks of that folder (datasets.RainyDataset, data/rain.py); never a source domain.
    ("cityscapes:" + root, "SPLIT[,foggy[=BETA]|rain][,caronly]") — the tools' `cityscapes:ROOT,SPLIT[,...]` — is Cityscapes as
    unpacked from its archives, the boxes taken from the instance-id maps (data/cityscapes.py); `device` is where such a set
    computes them (None: the HIP device when there is one, else the host; "cpu"), and means nothing to the other kinds."""
    first, second = spec
    if first.startswith(CITYSCAPES_PREFIX):
        from .cityscapes import CityscapesDataset, parse_options

        return CityscapesDataset(first[len(CITYSCAPES_PREFIX):], remove_images_without_annotations=is_train,
                                 transforms=transforms, is_source=is_source, decode_to_tensor=decode_to_tensor,
                                 device=device, **parse_options(second))
    if first.startswith(RAIN_PREFIX):
        from .rain import RainMasks

        if source_spec is None or is_rain_spec(source_spec):
            raise ValueError("a rain:MASKDIR dataset is built over the source dataset: source_spec is missing")
        inner = dataset_from_spec(source_spec, transforms, is_train, False, decode_to_tensor)
        return D.RainyDataset(inner, RainMasks(first[len(RAIN_PREFIX):]))
    if first.startswith("voc:"):
        return D.PascalVOCDataset(first[len("voc:"):], second, use_difficult=not is_train, transforms=transforms,
                                  is_source=is_source, decode_to_tensor=decode_to_tensor)
    return COCODataset(first, second, remove_images_without_annotations=is_train, transforms=transforms, is_source=is_source,
                       decode_to_tensor=decode_to_tensor)


def make_da_data_loaders(cfg, dataset_specs, is_distributed=False, start_iter=0, device_prep=False):
    """dataset_specs = {"source": (ann_file, root), "target": (...)[, "auxiliary": (...)]} (or `dataset_from_spec`'s VOC form;
    "auxiliary" may be ("rain:" + mask_dir, ""): the source images under synthesised rain)
    -> one loader per domain, iterated jointly by do_da_train (each carrying IMS_PER_BATCH // (2 * num_gpus) images per step).
    `device_prep=True`: the same batches, prepared on the device from decoded pixels (data/device_prep.py)."""
    tf = build_transforms(cfg, True)
    out = []
    for name in [n for n in ("source", "target", "auxiliary") if n in dataset_specs]:
        ds = dataset_from_spec(dataset_specs[name], tf, True, name == "source", decode_to_tensor=device_prep,
                               source_spec=dataset_specs["source"])
        collator = RawBatchCollator() if device_prep else BatchCollator(cfg.DATALOADER.SIZE_DIVISIBILITY)
        loader = _train_loader(cfg, ds, is_distributed, start_iter, collator)
        out.append(_device_prep_loader(cfg, loader, True) if device_prep else loader)
    if device_prep:
        from .device_prep import DevicePrepLoader

        DevicePrepLoader.consumed_jointly(out)
    return out


def make_triplet_data_loader(cfg, dataset_specs, is_distributed=False, start_iter=0, device_prep=False):
    """one loader over index-aligned (source, target, auxiliary) samples (build.py:23-63, 332-419); `device_prep` as above.
    A `rain:MASKDIR` auxiliary is built over the source dataset OBJECT: the triplet decodes the source image once and, under
    `device_prep`, uploads it once."""
    tf = build_transforms(cfg, True)
    ds = [dataset_from_spec(dataset_specs[n], tf, True, n == "source", decode_to_tensor=device_prep)
          for n in ("source", "target")]
    if is_rain_spec(dataset_specs["auxiliary"]):
        from .rain import RainMasks

        ds.append(D.RainyDataset(ds[0], RainMasks(dataset_specs["auxiliary"][0][len(RAIN_PREFIX):])))
        triplet = D.RainTripletDataset(ds)
    else:
        ds.append(dataset_from_spec(dataset_specs["auxiliary"], tf, True, False, decode_to_tensor=device_prep))
        triplet = TripletDataset(ds)
    collator = RawBatchCollator_triplet() if device_prep else BatchCollator_triplet(cfg.DATALOADER.SIZE_DIVISIBILITY)
    loader = _train_loader(cfg, triplet, is_distributed, start_iter, collator)
    return _device_prep_loader(cfg, loader, True) if device_prep else loader
