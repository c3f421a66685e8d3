"""PASCAL VOC AP on the device: the match launch (csrc/voc_match.hip) flag for flag and its IoU bit for bit against the plain
evaluator of tests/test_voc_eval.py, and the numbers end to end against the reference's recorded curves (yardsticks and
tolerances are stated there).

Shapes are the smallest at which the kernel can go wrong: pairs with 0 and 1 detections or ground truths, 257 detections
on 65 ground truths (past the 256-thread stride and the wave width), 1 and 16 thresholds, 1000 ground truths at 16 thresholds
(81000 B: LDS above the 48 KiB a launch gets without asking), one pair whose 2100 ground truths
at 16 thresholds (81 * 2100 B) no longer fit the 160 KiB of LDS and live in the workspace next to a small pair that does, an
IoU exactly at the threshold, identical ground truths, difficult ground truths claimed once, twice and in front of an easier
one."""
import os

import numpy as np
import pytest
import torch

from test_voc_eval import (AP_TOL, TWO_IMAGES, assert_ap_close, assert_curves_equal, fixture_boxlists, fixture_curves,
                           load_fixture, loop_ap, loop_voc, pred, truth, write_voc_tree)

pytestmark = pytest.mark.gpu


def device_flags(preds, gts, thresholds):
    from da_detect_amd.data.evaluation.voc import voc_eval

    packed = voc_eval.pack(preds, gts)
    match, n_pos, gt_index, iou_max = voc_eval.match(packed, thresholds)
    torch.cuda.synchronize()
    assert match.is_cuda and match.dtype == torch.int8 and tuple(match.shape) == (len(thresholds), len(packed.det_score))
    assert n_pos.dtype == torch.int32 and gt_index.dtype == torch.int32 and iou_max.dtype == torch.float32
    return packed, match.cpu(), n_pos.cpu(), gt_index.cpu(), iou_max.cpu()


def assert_flags_equal(preds, gts, thresholds, what):
    """match, n_pos, gt_index flag for flag; iou_max bit for bit"""
    loop = loop_voc(preds, gts, thresholds)
    packed, match, n_pos, gt_index, iou_max = device_flags(preds, gts, thresholds)
    assert n_pos.tolist() == loop["n_pos"].tolist(), what
    want = torch.from_numpy(loop["iou_max"])
    same = iou_max.view(torch.int32) == want.view(torch.int32)
    assert bool(same.all()), "%s: iou_max differs at %s: %s against %s" % (
        what, (~same).nonzero()[:5].flatten().tolist(), iou_max[~same][:5].tolist(), want[~same][:5].tolist())
    assert torch.equal(gt_index, torch.from_numpy(loop["gt_index"])), "%s: gt_index differs at %s" % (
        what, (gt_index != torch.from_numpy(loop["gt_index"])).nonzero()[:5].flatten().tolist())
    want = torch.from_numpy(loop["match"])
    assert torch.equal(match, want), "%s: match differs at %s" % (what, (match != want).nonzero()[:5].tolist())
    return loop, match


def test_edge_pairs():
    """one image per case; labels keep the cases apart inside an image where that is shorter"""
    box = [10, 10, 50, 40]
    cases = [
        ("D = 0", pred(np.zeros((0, 4)), [], []), truth([box], [1]), None),
        ("G = 0", pred([box, [0, 0, 5, 5]], [1, 1], [.9, .8]), truth(np.zeros((0, 4)), []), [[0, 0]]),
        ("D = G = 1", pred([box], [1], [.9]), truth([box], [1]), [[1]]),
        ("two detections on one ground truth", pred([box, [11, 10, 50, 40]], [1, 1], [.5, .9]), truth([box], [1]), [[1, 0]]),
        ("a difficult ground truth claimed twice", pred([box, [11, 10, 50, 40]], [1, 1], [.9, .5]), truth([box], [1], [1]),
         [[-1, -1]]),
        # the detection sits on the difficult box; the easier one next to it also passes 0.5, and is not fallen back to
        ("difficult best, easier one also passes", pred([[10, 10, 50, 40]], [1], [.9]),
         truth([[10, 10, 50, 40], [10, 10, 50, 30]], [1, 1], [1, 0]), [[-1]]),
        ("two identical ground truths", pred([box, box, box], [1, 1, 1], [.9, .8, .7]), truth([box, box], [1, 1]), [[1, 0, 0]]),
    ]
    for what, p, g, want in cases:
        loop, match = assert_flags_equal([p], [g], [.5], what)
        if want is not None:
            assert match.tolist() == want, what
    # all of them as one dataset, so that pairs of every kind share a launch
    assert_flags_equal([c[1] for c in cases], [c[2] for c in cases], [.5, .75], "all edge pairs in one launch")
    _, _, _, gt_index, _ = device_flags([cases[6][1]], [cases[6][2]], [.5])
    assert gt_index.tolist() == [0, 0, 0]                                         # the first index wins the tie
    _, _, _, gt_index, iou_max = device_flags([cases[1][1]], [cases[1][2]], [.5])
    assert gt_index.tolist() == [-1, -1] and iou_max.tolist() == [0.0, 0.0]


def test_iou_exactly_at_the_threshold():
    """(0, 0, 10, 1) on (0, 0, 4, 1): after x2 += 1, y2 += 1 and the "+1" of the areas, 6 * 3 = 18 of 36 + 18 - 18: exactly 0.5"""
    p, g = pred([[0, 0, 10, 1]], [1], [.9]), truth([[0, 0, 4, 1]], [1])
    loop, match = assert_flags_equal([p], [g], [.5, .75], "IoU at the threshold")
    _, _, _, _, iou_max = device_flags([p], [g], [.5, .75])
    assert iou_max.tolist() == [0.5] and match.tolist() == [[1], [0]]


def _crowded(rng, n_det, n_gt, label=1, size=(640, 480)):
    """n_gt ground truths on a jittered grid, n_det detections that are jittered copies of them (several per ground truth) or
    random boxes; about a fifth of the ground truths difficult; distinct scores"""
    gx, gy = rng.uniform(0, size[0] - 60, n_gt), rng.uniform(0, size[1] - 60, n_gt)
    gts = np.stack([gx, gy, gx + rng.uniform(8, 50, n_gt), gy + rng.uniform(8, 50, n_gt)], 1)
    pick = rng.integers(0, n_gt, n_det)
    dets = gts[pick] + rng.normal(0, 2.5, (n_det, 4))
    loose = rng.uniform(size=n_det) < .2
    dets[loose] = np.stack([rng.uniform(0, 300, loose.sum()), rng.uniform(0, 300, loose.sum()),
                            rng.uniform(310, 600, loose.sum()), rng.uniform(310, 470, loose.sum())], 1)
    dets[:, 2:] = np.maximum(dets[:, 2:], dets[:, :2] + 1)
    scores = (rng.permutation(n_det) + 1.0) / (n_det + 1)
    return (pred(dets, [label] * n_det, scores, size), truth(gts, [label] * n_gt, rng.uniform(size=n_gt) < .2, size))


@pytest.mark.parametrize("thresholds", [[.5], [.3 + .04 * k for k in range(16)]], ids=["T1", "T16"])
def test_past_the_thread_stride_and_the_wave_width(thresholds):
    p, g = _crowded(np.random.default_rng(3), 257, 65)
    loop, match = assert_flags_equal([p], [g], thresholds, "D = 257, G = 65, T = %d" % len(thresholds))
    assert {-1, 0, 1} <= set(match.flatten().tolist())
    if len(thresholds) > 1:
        assert (match[0] != match[-1]).any()


def test_lds_above_the_default_limit():
    """G = 1000 at T = 16 is 81000 B of LDS: above the 48 KiB a launch gets without asking, below the 160 KiB of a CU"""
    p, g = _crowded(np.random.default_rng(4), 120, 1000, size=(2048, 1024))
    loop, match = assert_flags_equal([p], [g], [.3 + .04 * k for k in range(16)], "D = 120, G = 1000, T = 16")
    assert {-1, 0, 1} <= set(match.flatten().tolist())


def test_workspace_fallback_next_to_an_lds_pair():
    from da_detect_amd import _C

    rng = np.random.default_rng(5)
    thresholds = [.3 + .04 * k for k in range(16)]
    big_p, big_g = _crowded(rng, 300, 2100, label=2, size=(2048, 1024))
    small_p, small_g = _crowded(rng, 40, 9, label=1, size=(2048, 1024))
    p = pred(np.concatenate([small_p.bbox.numpy(), big_p.bbox.numpy()]), [1] * 40 + [2] * 300,
             np.concatenate([small_p.get_field("scores").numpy(), big_p.get_field("scores").numpy() * .5]), (2048, 1024))
    g = truth(np.concatenate([small_g.bbox.numpy(), big_g.bbox.numpy()]), [1] * 9 + [2] * 2100,
              np.concatenate([small_g.get_field("difficult").numpy(), big_g.get_field("difficult").numpy()]), (2048, 1024))
    lds_only = _C.voc_match_workspace_bytes([0, 40], [0, 9], 40, 9, 16)
    assert _C.voc_match_workspace_bytes([0, 40, 340], [0, 9, 2109], 340, 2109, 16) >= lds_only + 81 * 2100
    loop, match = assert_flags_equal([p], [g], thresholds, "G = 2100 at T = 16 in the workspace")
    assert {-1, 0, 1} <= set(match[:, 40:].flatten().tolist()) and {0, 1} <= set(match[:, :40].flatten().tolist())


@pytest.fixture(scope="module")
def fixture():
    return load_fixture()


def test_fixture_end_to_end(fixture):
    """the reference's recorded curves and APs, from this package's entry points"""
    from da_detect_amd.data.evaluation.voc import voc_eval

    preds, gts = fixture_boxlists(fixture)
    thresholds = fixture["thresholds"].tolist()
    assert thresholds == [.5, .75]
    prec, rec = voc_eval.calc_detection_voc_prec_rec(gt_boxlists=gts, pred_boxlists=preds, iou_thresh=thresholds)
    for t, thr in enumerate(thresholds):
        want_prec, want_rec = fixture_curves(fixture, t)
        assert_curves_equal(prec[t], want_prec, "prec at IoU %.2f" % thr)
        assert_curves_equal(rec[t], want_rec, "rec at IoU %.2f" % thr)
        single = voc_eval.calc_detection_voc_prec_rec(gts, preds, iou_thresh=thr)
        assert_curves_equal(single[0], want_prec, "prec at IoU %.2f, alone" % thr)
        assert_curves_equal(single[1], want_rec, "rec at IoU %.2f, alone" % thr)
        for m, use_07 in enumerate((True, False)):
            what = "IoU %.2f %s" % (thr, "11-point" if use_07 else "area")
            result = voc_eval.eval_detection_voc(preds, gts, iou_thresh=thr, use_07_metric=use_07)
            assert sorted(result) == ["ap", "map"] and result["ap"].dtype == np.float64
            assert_ap_close(result["ap"], fixture["ap"][t, m], what)
            print(what, "map %.12f reference %.12f" % (result["map"], fixture["map"][t, m]))
            assert abs(result["map"] - fixture["map"][t, m]) <= AP_TOL
    for m, use_07 in enumerate((True, False)):
        result = voc_eval.eval_detection_voc(preds, gts, iou_thresh=thresholds, use_07_metric=use_07)
        assert_ap_close(result["ap_by_iou"], fixture["ap"][:, m], "both thresholds in one launch, use_07_metric=%s" % use_07)
        assert_ap_close(result["ap"], fixture["ap"][0, m], "first threshold")
        assert abs(result["map"] - fixture["map"][0, m]) <= AP_TOL
    assert_flags_equal(preds, gts, thresholds, "fixture flags")


def test_random_set():
    """60 images, 6 classes, a few thousand detections with distinct scores: flags, curves and APs against the plain evaluator"""
    from da_detect_amd.data.evaluation.voc import voc_eval

    rng = np.random.default_rng(17)
    preds, gts = [], []
    for i in range(60):
        parts = [_crowded(rng, int(rng.integers(10, 30)), int(rng.integers(1, 6)), label=int(k))
                 for k in rng.choice(np.arange(1, 7), size=int(rng.integers(2, 5)), replace=False)]
        boxes, labels = np.concatenate([p.bbox.numpy() for p, _ in parts]), np.concatenate([p.get_field("labels").numpy() for p, _ in parts])
        stray = rng.uniform(size=len(labels)) < .1                     # some detections carry another class's label
        labels[stray] = rng.integers(1, 7, int(stray.sum()))
        preds.append(pred(boxes, labels, np.zeros(len(labels))))
        gts.append(truth(np.concatenate([g.bbox.numpy() for _, g in parts]), np.concatenate([g.get_field("labels").numpy() for _, g in parts]),
                         np.concatenate([g.get_field("difficult").numpy() for _, g in parts])))
    total = sum(len(p) for p in preds)
    scores = ((rng.permutation(total) + 1.0) / (total + 1)).astype(np.float32)
    assert 2000 <= total <= 6000 and len(np.unique(scores)) == total
    at = 0
    for p in preds:
        p.add_field("scores", torch.from_numpy(scores[at:at + len(p)]))
        at += len(p)
    thresholds = [.5, .7]
    loop, match = assert_flags_equal(preds, gts, thresholds, "random set")
    assert {-1, 0, 1} <= set(match.flatten().tolist())
    prec, rec = voc_eval.calc_detection_voc_prec_rec(gts, preds, iou_thresh=thresholds)
    for t in range(2):
        assert_curves_equal(prec[t], loop["prec"][t], "prec")
        assert_curves_equal(rec[t], loop["rec"][t], "rec")
    for use_07 in (True, False):
        result = voc_eval.eval_detection_voc(preds, gts, iou_thresh=thresholds, use_07_metric=use_07)
        want = np.stack([loop_ap(loop["prec"][t], loop["rec"][t], use_07) for t in range(2)])
        assert_ap_close(result["ap_by_iou"], want, "random set, use_07_metric=%s" % use_07)
        assert abs(result["map"] - np.nanmean(want[0])) <= AP_TOL and 0.0 < result["map"] < 1.0


def _voc_predictions():
    """image 1 of TWO_IMAGES at twice its size: the car exactly, the dog exactly, a person on the difficult box, a stray car;
    image 2: nothing"""
    first = pred([[0, 0, 39, 59], [8, 10, 127, 95], [18, 22, 79, 87], [60, 2, 100, 40]], [7, 12, 15, 7], [.9, .8, .7, .6], (128, 96))
    return [first, pred(np.zeros((0, 4)), [], [], (50, 40))]


def test_do_voc_evaluation_writes_result_txt(tmp_path):
    from da_detect_amd.data.datasets import PascalVOCDataset
    from da_detect_amd.data.evaluation import evaluate

    dataset = PascalVOCDataset(write_voc_tree(tmp_path, TWO_IMAGES), "test", use_difficult=True)
    out = tmp_path / "out"
    out.mkdir()
    result = evaluate(dataset, _voc_predictions(), str(out), box_only=False, iou_types=("bbox",), expected_results=(),
                      expected_results_sigma_tol=4)
    # image 2 is skipped with its bicycle, so label 2 never occurs; car: 1 of 1 found first, then a false positive; dog: found;
    # person: only a difficult box, no positives
    ap = result["ap"]
    assert ap.shape == (16,) and ap[7] == pytest.approx(1.0, abs=AP_TOL) and ap[12] == pytest.approx(1.0, abs=AP_TOL)
    assert np.isnan(ap[[0, 2, 15]]).all() and result["map"] == pytest.approx(1.0, abs=AP_TOL)
    lines = open(str(out / "result.txt")).read().splitlines()
    assert lines[0] == "mAP: 1.0000" and len(lines) == 16
    assert lines[7] == "{:<16}: {:.4f}".format("car", 1.0) and lines[2] == "{:<16}: {:.4f}".format("bicycle", float("nan"))
    # the area metric at a threshold the stray car's IoU does not matter for, through evaluate's keywords
    other = evaluate(dataset, _voc_predictions(), None, use_07_metric=False, iou_thresh=[.5, .9])
    assert other["ap_by_iou"].shape == (2, 16) and other["ap"][7] == pytest.approx(1.0, abs=AP_TOL)


def test_empty_predictions_everywhere(tmp_path):
    from da_detect_amd.data.datasets import PascalVOCDataset
    from da_detect_amd.data.evaluation.voc import voc_eval

    dataset = PascalVOCDataset(write_voc_tree(tmp_path, TWO_IMAGES), "test", use_difficult=True)
    nothing = [pred(np.zeros((0, 4)), [], [], (64, 48)), pred(np.zeros((0, 4)), [], [], (50, 40))]
    result = voc_eval.do_voc_evaluation(dataset, nothing, str(tmp_path))
    assert result["ap"].shape == (0,) and np.isnan(result["map"])
    assert open(os.path.join(str(tmp_path), "result.txt")).read() == "mAP: nan\n"
    # images kept but without detections (eval_detection_voc itself skips nothing): every class with positives scores 0
    gts = [dataset.get_groundtruth(0), dataset.get_groundtruth(1)]
    for use_07 in (True, False):
        result = voc_eval.eval_detection_voc(nothing, gts, use_07_metric=use_07)
        assert result["ap"][[2, 7, 12]].tolist() == [0.0, 0.0, 0.0] and np.isnan(result["ap"][15]) and result["map"] == 0.0


def test_score_tool_voc_metric_on_a_coco_dataset(tmp_path):
    """tools/score_net_da.py --metric voc07 on COCO-format data: the crowd annotation counts as difficult (the detection on it
    is neither hit nor miss), the others score as VOC scores them"""
    import json
    import subprocess
    import sys

    from da_detect_amd.data.datasets import COCODataset

    path = os.path.join(str(tmp_path), "ann.json")
    with open(path, "w") as f:
        json.dump({"images": [{"id": 5, "file_name": "a.png", "width": 100, "height": 80}],
                   "annotations": [{"id": 1, "image_id": 5, "category_id": 26, "bbox": [10, 20, 30, 40], "area": 1200, "iscrowd": 0},
                                   {"id": 2, "image_id": 5, "category_id": 26, "bbox": [60, 10, 30, 30], "area": 900, "iscrowd": 1},
                                   {"id": 3, "image_id": 5, "category_id": 24, "bbox": [0, 0, 20, 20], "area": 400, "iscrowd": 0}],
                   "categories": [{"id": 24, "name": "person"}, {"id": 26, "name": "car"}]}, f)
    dataset = COCODataset(path, str(tmp_path), remove_images_without_annotations=False)
    # best first: on the crowd car (-1), far from everything (0), on the car (1); the person is missed
    predictions = [pred([[60, 10, 89, 39], [40, 60, 50, 70], [10, 20, 39, 59]], [2, 2, 2], [.9, .8, .7], (100, 80))]
    saved = os.path.join(str(tmp_path), "predictions.pth")
    torch.save(predictions, saved)
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "score_net_da.py")
    res = subprocess.run([sys.executable, tool, "--dataset", path + "," + str(tmp_path), "--predictions", saved, "--metric", "voc07"],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    # car: flags (-1, 0, 1) -> prec (nan, 0, 1/2), rec (0, 0, 1): 11 points of 1/2.  As a plain miss the crowd box would cost more.
    want_car = sum([.5 / 11] * 11)
    lines = open(os.path.join(str(tmp_path), "result.txt")).read().splitlines()
    assert lines == ["mAP: %.4f" % (want_car / 2), "{:<16}: {:.4f}".format("person", 0.0), "{:<16}: {:.4f}".format("car", want_car)]
    assert "mAP: %.4f" % (want_car / 2) in res.stderr
    from da_detect_amd.data.evaluation.voc import do_voc_evaluation

    direct = do_voc_evaluation(dataset, predictions, None)
    assert direct["ap"][1] == 0.0 and abs(direct["ap"][2] - want_car) <= AP_TOL and np.isnan(direct["ap"][0])


def test_score_tool_evaluates_and_scores_a_voc_layout_set(tmp_path):
    """tools/score_net_da.py --dataset voc:DIR,SPLIT --config-file: the evaluation pass (seeded random weights, tiny images) and
    the VOC scoring in one command"""
    import subprocess
    import sys

    images = [("a", 192, 96, [("car", 10, 10, 80, 60, 0), ("person", 100, 20, 150, 90, 1)]), ("b", 160, 96, [("dog", 5, 5, 90, 90, 0)])]
    tree = write_voc_tree(tmp_path / "VOCtiny", images)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "out")
    os.makedirs(out)
    run = [sys.executable, os.path.join(root, "tools", "score_net_da.py"), "--dataset", "voc:" + tree + ",test", "--config-file",
           os.path.join(root, "configs/da_faster_rcnn/e2e_da_faster_rcnn_R_50_C4_cityscapes_to_foggy_cityscapes.yaml"),
           "--output-dir", out, "--metric", "voc12", "DATALOADER.NUM_WORKERS", "0", "INPUT.MIN_SIZE_TEST", "96",
           "INPUT.MAX_SIZE_TEST", "192", "MODEL.WEIGHT", "", "MODEL.ROI_BOX_HEAD.NUM_CLASSES", "21",
           "MODEL.ROI_HEADS.SCORE_THRESH", "0.0"]
    res = subprocess.run(run, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    where = os.path.join(out, "inference", "VOCtiny_test")
    predictions = torch.load(os.path.join(where, "predictions.pth"), weights_only=False)
    assert len(predictions) == 2 and sum(len(p) for p in predictions) > 0
    lines = open(os.path.join(where, "result.txt")).read().splitlines()
    assert lines[0].startswith("mAP: ") and len(lines) >= 2 and all(": " in line for line in lines)
    assert lines[0] in res.stderr


def test_malformed_offsets_are_refused_before_the_launch():
    from da_detect_amd import _C, _lib

    dev = torch.device("cuda")
    det = torch.tensor([[0., 0., 9., 9.], [0., 0., 9., 4.], [50., 50., 54., 54.]], device=dev)
    gt = torch.tensor([[0., 0., 9., 9.], [50., 50., 54., 54.]], device=dev)
    hard = torch.zeros(2, dtype=torch.uint8, device=dev)
    for det_off, gt_off in (([0, 2, 1], [0, 1, 2]), ([0, 2, 10 ** 6], [0, 1, 2]), ([0, 2, 3], [0, 5, 2]), ([1, 2, 3], [0, 1, 2]),
                            ([0, 2, 3], [0, 1, 1]), ([0, -1, 3], [0, 1, 2]), ([0, 2, 3], [0, 1])):
        with pytest.raises(_lib.DadetError) as err:
            _C.voc_match(det, gt, hard, det_off, gt_off, [.5])
        assert "status -1" in str(err.value) or "pairs + 1" in str(err.value)
    for thresholds in ([], [.5] * 17):
        with pytest.raises(_lib.DadetError, match="status -1"):
            _C.voc_match(det, gt, hard, [0, 2, 3], [0, 1, 2], thresholds)
    # nothing faulted: the well-formed table still runs, and gives the obvious answer
    match, n_pos, gt_index, iou_max = _C.voc_match(det, gt, hard, [0, 2, 3], [0, 1, 2], [.5, .75])
    torch.cuda.synchronize()
    assert n_pos.tolist() == [1, 1] and gt_index.tolist() == [0, 0, 0]
    assert match.tolist() == [[1, 0, 1], [1, 0, 1]]          # the exact box takes the ground truth; the half box comes second
    assert iou_max[0].item() == 1.0 and iou_max[2].item() == 1.0


def test_both_matchers_share_a_stream():
    """The two matchers raise the LDS limit per kernel and upload their tables through the same code (csrc/pair_tables.h).  On
    one stream, in this order: VOC with 81000 B of LDS, a small COCO pair, COCO with a 100 x 150 matrix (120000 B, above the
    48 KiB a launch gets without asking), a small VOC pair — every output of all four against the plain loops, exactly."""
    from da_detect_amd.data.evaluation.coco import box_ap
    from da_detect_amd.data.evaluation.voc import voc_eval
    from test_coco_eval import ListDataset, _ann, _det, _images, flags_in_packed_order, loop_box_ap

    sixteen = [.3 + .04 * k for k in range(16)]
    rng = np.random.default_rng(6)
    voc_big = _crowded(rng, 120, 1000, size=(2048, 1024))
    voc_small = (pred([[0, 0, 9, 9], [0, 0, 9, 4], [50, 50, 54, 54]], [1, 1, 1], [.9, .8, .7]),
                 truth([[0, 0, 9, 9], [50, 50, 54, 54]], [1, 1]))
    coco_small = (ListDataset(_images(1), [_ann(10, 1, [0, 0, 10, 10]), _ann(10, 1, [50, 50, 5, 5])], [1]),
                  [_det(10, 1, [0, 0, 10, 10], .9), _det(10, 1, [0, 0, 10, 5], .8), _det(10, 1, [50, 50, 5, 5], .7)])
    gts = [[float(np.round(v, 1)) for v in (rng.uniform(0, 900), rng.uniform(0, 900), side, side * rng.uniform(.6, 1.4))]
           for side in ([rng.uniform(6, 30), rng.uniform(34, 90), rng.uniform(100, 220)][j % 3] for j in range(150))]
    dets = []
    for j in range(100):
        x, y, w, h = gts[int(rng.integers(150))]
        s = rng.uniform(.0, .2)
        box = [x + w * rng.normal(0, s), y + h * rng.normal(0, s), w * (1 + rng.normal(0, s)), h * (1 + rng.normal(0, s))]
        dets.append(_det(10, 1, [float(np.float32(v)) for v in box], (j + 1) / 128))
    coco_big = (ListDataset(_images(1), [_ann(10, 1, b, crowd=1 if j % 7 == 6 else 0) for j, b in enumerate(gts)], [1]), dets)

    voc_packed = [voc_eval.pack([p], [g]) for p, g in (voc_big, voc_small)]
    coco_packed = [box_ap.pack(records, dataset) for dataset, records in (coco_small, coco_big)]
    assert voc_packed[0].gt_off.tolist() == [0, 1000] and coco_packed[1].det_off.tolist() == [0, 100]
    assert coco_packed[1].gt_off.tolist() == [0, 150] and coco_packed[0].det_off.tolist() == [0, 3]
    got = [voc_eval.match(voc_packed[0], sixteen), box_ap.match(coco_packed[0]), box_ap.match(coco_packed[1]),
           voc_eval.match(voc_packed[1], [.5, .75])]
    torch.cuda.synchronize()

    for (p, g), thresholds, (match, n_pos, gt_index, iou_max) in ((voc_big, sixteen, got[0]), (voc_small, [.5, .75], got[3])):
        loop = loop_voc([p], [g], thresholds)
        assert n_pos.tolist() == loop["n_pos"].tolist()
        assert torch.equal(iou_max.cpu().view(torch.int32), torch.from_numpy(loop["iou_max"]).view(torch.int32))
        assert torch.equal(gt_index.cpu(), torch.from_numpy(loop["gt_index"]))
        assert torch.equal(match.cpu(), torch.from_numpy(loop["match"]))
    assert got[3][0].tolist() == [[1, 0, 1], [1, 0, 1]] and {-1, 0, 1} <= set(got[0][0].flatten().tolist())
    for (dataset, records), packed, (matched, ignored, npig) in ((coco_small, coco_packed[0], got[1]),
                                                                  (coco_big, coco_packed[1], got[2])):
        want_m, want_i, want_n = flags_in_packed_order(packed, loop_box_ap(records, dataset))
        assert torch.equal(npig.cpu(), want_n)
        assert torch.equal(matched.cpu(), want_m) and torch.equal(ignored.cpu(), want_i)
    assert got[1][0][:, 0, :].tolist() == [[1, 0, 1]] * 10
    assert 0 < int(got[2][0].sum()) < got[2][0].numel() and 0 < int(got[2][1].sum()) < got[2][1].numel()
