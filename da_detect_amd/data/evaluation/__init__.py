"""Dataset-specific scoring of a finished inference pass (reference: maskrcnn_benchmark/data/datasets/evaluation/__init__.py).
`compat.install()` answers for this package under the reference's path, `maskrcnn_benchmark.data.datasets.evaluation`."""
from .. import datasets
from .coco import coco_evaluation


def _is_coco(dataset):
    if isinstance(dataset, datasets.COCODataset):
        return True
    return isinstance(dataset, datasets.ConcatDataset) and len(dataset.datasets) > 0 and all(
        _is_coco(d) for d in dataset.datasets)


def evaluate(dataset, predictions, output_folder, **kwargs):
    """`predictions`: one BoxList per image of `dataset`; `output_folder`: where the scorer leaves its files (None: nowhere);
    further keyword arguments go to the scorer.  COCO-style datasets (and concatenations of them) are the only kind here."""
    if _is_coco(dataset):
        return coco_evaluation(dataset=dataset, predictions=predictions, output_folder=output_folder, **kwargs)
    raise NotImplementedError("Unsupported dataset type {}.".format(dataset.__class__.__name__))
