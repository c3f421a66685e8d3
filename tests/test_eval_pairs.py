"""What the COCO and the VOC scorer share (da_detect_amd/data/evaluation/pairs.py), on inputs small enough to write the answer
down: the offset tables of the (image, class) pairs, and the padded per-class grid of `accumulate`.  No device."""
import numpy as np
import torch

from test_coco_eval import ListDataset, _ann, _det, _images
from test_voc_eval import pred, truth

# 3 images x 3 classes, key = image * 3 + class.  Image 0: class 0 has detections only, class 1 ground truth only.  Image 1 is
# empty.  Image 2: class 0 has three equal scores and one ground truth, class 2 five detections (two of them tied for the best)
# and two ground truths, in interleaved record order.
DET_IMAGE = [0, 0, 2, 2, 2, 2, 2, 2, 2, 2]
DET_CLASS = [0, 0, 2, 0, 2, 0, 2, 2, 0, 2]
DET_SCORE = [.5, .875, .125, .25, .75, .25, .375, .75, .25, .1875]       # exact in float32
GT_IMAGE = [0, 0, 2, 2, 2]
GT_CLASS = [1, 1, 2, 0, 2]
PAIR_KEY = [0, 1, 6, 8]
GT_ORDER, GT_OFF = [0, 1, 3, 2, 4], [0, 0, 2, 3, 5]
DET_ORDER, DET_OFF = [1, 0, 3, 5, 8, 4, 7, 6, 9, 2], [0, 2, 2, 5, 10]
DET_ORDER_CUT2, DET_OFF_CUT2 = [1, 0, 3, 5, 4, 7], [0, 2, 2, 4, 6]


def _keys():
    return (np.array(DET_IMAGE) * 3 + np.array(DET_CLASS), np.array(DET_SCORE, dtype=np.float64),
            np.array(GT_IMAGE) * 3 + np.array(GT_CLASS))


def _assert_tables(got, order, det_off):
    det_order, gt_order, pair_key, got_det_off, gt_off = got
    assert pair_key.tolist() == PAIR_KEY
    assert det_order.tolist() == order and got_det_off.tolist() == det_off and got_det_off.dtype == np.int32
    assert gt_order.tolist() == GT_ORDER and gt_off.tolist() == GT_OFF and gt_off.dtype == np.int32


def test_pair_tables_by_hand():
    from da_detect_amd.data.evaluation import pairs

    key, score, gkey = _keys()
    _assert_tables(pairs.pair_tables(key, score, gkey), DET_ORDER, DET_OFF)
    _assert_tables(pairs.pair_tables(key, score, gkey, cut=2), DET_ORDER_CUT2, DET_OFF_CUT2)
    cut = pairs.pair_tables(key, score, gkey, cut=2)[0]
    assert cut[4:6].tolist() == [4, 7]                    # of .125 .75 .375 .75 .1875: the two best, in record order
    assert cut[2:4].tolist() == [3, 5]                    # of three equal scores: the first two records
    # nothing at all: one offset each, no pair
    none = pairs.pair_tables(np.zeros(0, np.int64), np.zeros(0), np.zeros(0, np.int64), cut=2)
    assert [len(a) for a in none] == [0, 0, 0, 1, 1] and none[3].tolist() == [0] and none[4].tolist() == [0]


def test_pair_tables_are_what_the_scorers_pack():
    """box x of detection / ground truth i is i, so the packed boxes spell the orders out"""
    from da_detect_amd.data.evaluation import pairs
    from da_detect_amd.data.evaluation.coco import box_ap
    from da_detect_amd.data.evaluation.voc import voc_eval

    key, score, gkey = _keys()
    preds, gts = [], []
    for image in range(3):
        d = [i for i in range(len(DET_IMAGE)) if DET_IMAGE[i] == image]
        g = [i for i in range(len(GT_IMAGE)) if GT_IMAGE[i] == image]
        preds.append(pred(np.array([[i, 0, i + 5, 5] for i in d]).reshape(-1, 4), [DET_CLASS[i] for i in d],
                          [DET_SCORE[i] for i in d]))
        gts.append(truth(np.array([[i, 0, i + 5, 5] for i in g]).reshape(-1, 4), [GT_CLASS[i] for i in g]))
    p = voc_eval.pack(preds, gts)
    assert p.n_class == 3
    _assert_tables((p.det_box[:, 0].astype(np.int64), p.gt_box[:, 0].astype(np.int64), p.pair_key, p.det_off, p.gt_off),
                   DET_ORDER, DET_OFF)
    want = pairs.pair_tables(key, score, gkey)
    assert p.det_score.tolist() == score[want[0]].tolist() and p.det_label.tolist() == np.array(DET_CLASS)[want[0]].tolist()

    dataset = ListDataset(_images(3), [_ann(10 + GT_IMAGE[i], 1 + GT_CLASS[i], [i, 0, 5, 5]) for i in range(len(GT_IMAGE))],
                          [1, 2, 3])
    records = [_det(10 + DET_IMAGE[i], 1 + DET_CLASS[i], [i, 0, 5, 5], DET_SCORE[i]) for i in range(len(DET_IMAGE))]
    c = box_ap.pack(records, dataset)
    want = pairs.pair_tables(key, score, gkey, cut=box_ap.MAX_DETS)
    _assert_tables(want, DET_ORDER, DET_OFF)              # nothing here reaches the cut of 100
    _assert_tables((c.det_box[:, 0].astype(np.int64), c.gt_box[:, 0].astype(np.int64), c.pair_key, c.det_off, c.gt_off),
                   DET_ORDER, DET_OFF)
    assert c.det_score.tolist() == score[want[0]].tolist() and c.det_cat.tolist() == np.array(DET_CLASS)[want[0]].tolist()


def test_class_grid_and_class_sum_by_hand():
    """K = 3, class 1 empty; packed order is image, class, score: image 0 holds (class 0, .5), (class 2, .75), (class 2, .5),
    image 1 holds (class 0, .75), (class 2, .5) — the two .5 of class 2 tie across images and keep the image order"""
    from da_detect_amd.data.evaluation import pairs

    score = np.array([.5, .75, .5, .75, .5])
    label = np.array([0, 2, 2, 0, 2], dtype=np.int64)
    where, counts, L = pairs.class_grid(score, label, 3, torch.device("cpu"))
    assert L == 3 and counts.tolist() == [2, 0, 3] and counts.dtype == np.int64
    assert where.dtype == torch.int64 and where.tolist() == [[3, 0, 5], [5, 5, 5], [1, 2, 4]]      # 5 = n: the padding column
    where, counts, L = pairs.class_grid(np.zeros(0), np.zeros(0, np.int64), 2, torch.device("cpu"))
    assert L == 1 and counts.tolist() == [0, 0] and where.tolist() == [[0], [0]]
    where, counts, L = pairs.class_grid(np.zeros(0), np.zeros(0, np.int64), 0, torch.device("cpu"))
    assert L == 1 and len(counts) == 0 and tuple(where.shape) == (0, 1)

    pair_key = np.array([0, 2, 3, 5])                     # classes 0, 2, 0, 2
    total = pairs.class_sum(pair_key, 3, torch.tensor([1, 2, 3, 4], dtype=torch.int32), torch.device("cpu"))
    assert total.dtype == torch.int64 and total.tolist() == [4, 0, 6]
    total = pairs.class_sum(pair_key, 3, torch.tensor([[1, 0], [2, 1], [3, 0], [4, 1]], dtype=torch.int32), torch.device("cpu"))
    assert total.tolist() == [[4, 0], [0, 0], [6, 2]]
    assert pairs.class_sum(np.zeros(0, np.int64), 0, torch.zeros(0, dtype=torch.int32), torch.device("cpu")).tolist() == []
