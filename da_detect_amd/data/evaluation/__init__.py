"""Dataset-specific scoring of a finished inference pass (reference: maskrcnn_benchmark/data/datasets/evaluation/__init__.py).
`compat.install()` answers for this package under the reference's path, `maskrcnn_benchmark.data.datasets.evaluation`."""
from .. import datasets
from .coco import coco_evaluation
from .voc import voc_evaluation


def _is_kind(dataset, kind):
    if isinstance(dataset, kind):
        return True
    return isinstance(dataset, datasets.ConcatDataset) and len(dataset.datasets) > 0 and all(
        _is_kind(d, kind) for d in dataset.datasets)


def _is_coco(dataset):
    return _is_kind(dataset, datasets.COCODataset)


def evaluate(dataset, predictions, output_folder, **kwargs):
    """`predictions`: one BoxList per image of `dataset`; `output_folder`: where the scorer leaves its files (None: nowhere);
    further keyword arguments go to the scorer.  COCO-style datasets go to the COCO scorer, PASCAL VOC ones to the VOC scorer
    (which also takes `iou_thresh=` and `use_07_metric=`); so do concatenations of one kind."""
    if _is_coco(dataset):
        return coco_evaluation(dataset=dataset, predictions=predictions, output_folder=output_folder, **kwargs)
    if _is_kind(dataset, datasets.PascalVOCDataset):
        return voc_evaluation(dataset=dataset, predictions=predictions, output_folder=output_folder, **kwargs)
    raise NotImplementedError("Unsupported dataset type {}.".format(dataset.__class__.__name__))
