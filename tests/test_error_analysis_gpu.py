"""Error breakdown of detections on the device (csrc/error_match.hip): every output array of the launch against
the plain loop evaluator of tests/_error_cases.py — kinds, defining ground truths, fix flags, ground-truth states flag for
flag, `iou_same` / `iou_other` bit for bit — the TP / ignored flags against the existing VOC matcher, `summarise` against
the VOC scorer and the float64 loop, and the two tools end to end.

Shapes are the smallest at which the kernel can go wrong: images with 0 and 1 detections or ground truths and one image per
branch of the rule, IoU exactly at both thresholds, 257 detections on 65 ground truths of 3 classes (past the 256-thread
stride and the wave width), 1500 ground truths (49.5 KB of LDS: above the 48 KiB a launch gets without asking), and 5000
ground truths (165 000 B: no longer in the 160 KiB of LDS, so in the workspace) next to a 9-ground-truth image that stays in
LDS.  Tolerances are those of tests/test_error_analysis_host.py: integers and IoU bits equal, AP figures within AP_TOL."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _error_cases as cases
from _error_cases import BKG, CLS, COVERED, DETECTED, DIFFICULT, IGNORED, LOC, MISSED, TP
from test_error_analysis_host import assert_summary_close, load_tool
from test_voc_eval import AP_TOL, ROOT, TWO_IMAGES, assert_ap_close, fixture_boxlists, load_fixture, pred, write_voc_tree

pytestmark = pytest.mark.gpu
ARRAYS = ("det_kind", "det_gt", "iou_same", "iou_other", "det_fix", "gt_state", "gt_det")


def device_outputs(preds, gts, pos=0.5, bg=0.1):
    from da_detect_amd.data.evaluation import errors

    packed = errors.pack(preds, gts)
    out = errors.match(packed, pos, bg)
    torch.cuda.synchronize()
    assert all(t.is_cuda for t in out)
    assert [t.dtype for t in out] == [torch.uint8, torch.int32, torch.float32, torch.float32, torch.uint8, torch.uint8, torch.int32]
    return packed, out


def assert_outputs_equal(preds, gts, what, pos=0.5, bg=0.1, loop=None):
    """all seven arrays of the launch against the loop: flags equal, IoUs equal as bit patterns"""
    loop = loop if loop is not None else cases.loop_errors(preds, gts, pos, bg)
    packed, out = device_outputs(preds, gts, pos, bg)
    assert packed.det_off.tolist() == loop["det_off"].tolist() and packed.gt_off.tolist() == loop["gt_off"].tolist(), what
    for name, got in zip(ARRAYS, out):
        got, want = got.cpu(), torch.from_numpy(loop[name])
        assert got.shape == want.shape, (what, name, got.shape, want.shape)
        if want.dtype == torch.float32:
            got, want = got.view(torch.int32), want.view(torch.int32)
        differ = (got != want).nonzero().flatten()
        assert len(differ) == 0, "%s: %s differs at %s: %s against %s" % (
            what, name, differ[:5].tolist(), out[ARRAYS.index(name)].cpu()[differ[:5]].tolist(), loop[name][differ[:5].numpy()].tolist())
    return packed, out, loop


def test_edge_images():
    edge = cases.edge_images()
    for what, p, g, kinds, fixes in edge:
        packed, out, loop = assert_outputs_equal([p], [g], what)
        assert out.det_kind.tolist() == kinds and out.det_fix.tolist() == fixes, what
    # all of them in one launch, so that images of every kind share it
    packed, out, loop = assert_outputs_equal([c[1] for c in edge], [c[2] for c in edge], "all edge images in one launch")
    assert out.det_kind.tolist() == sum([c[3] for c in edge], []) and out.det_fix.tolist() == sum([c[4] for c in edge], [])
    _, out = device_outputs([edge[1][1]], [edge[1][2]])                          # no ground truth
    assert out.det_kind.tolist() == [BKG, BKG] and out.det_gt.tolist() == [-1, -1]
    assert out.iou_same.tolist() == [0.0, 0.0] and out.iou_other.tolist() == [0.0, 0.0]
    _, out = device_outputs([edge[0][1]], [edge[0][2]])                          # no detections
    assert out.gt_state.tolist() == [MISSED] and out.gt_det.tolist() == [-1] and out.det_kind.numel() == 0
    _, out = device_outputs([edge[3][1]], [edge[3][2]])                          # identical ground truths: the first wins the tie
    assert out.det_gt.tolist() == [0, 0, 0] and out.gt_state.tolist() == [DETECTED, MISSED] and out.gt_det.tolist() == [0, -1]
    _, out = device_outputs([edge[6][1]], [edge[6][2]])                          # Dupe-eligible and Cls-eligible -> Cls
    assert out.det_gt.tolist() == [0, 1] and out.gt_state.tolist() == [DETECTED, COVERED]
    _, out = device_outputs([edge[8][1]], [edge[8][2]])                          # a Loc and a Cls claim separately
    assert out.det_gt.tolist() == [0, 0] and out.gt_state.tolist() == [COVERED]
    _, out = device_outputs([edge[5][1]], [edge[5][2]])                          # the difficult one in front of the easier one
    assert out.det_gt.tolist() == [0] and out.gt_state.tolist() == [DIFFICULT, MISSED]


def test_iou_exactly_at_both_thresholds():
    """the boxes and their IoU values are worked out in `threshold_images`: 0.5 is a TP, float32 0.1 a Loc (both thresholds
    are inclusive), 0.09 background"""
    images = cases.threshold_images()
    for what, p, g, kind, iou in images:
        packed, out, loop = assert_outputs_equal([p], [g], what)
        assert out.det_kind.tolist() == [kind], what
        assert out.iou_same.cpu().view(torch.int32).tolist() == [int(np.float32(iou).view(np.int32))], (what, out.iou_same.tolist())
    assert_outputs_equal([c[1] for c in images], [c[2] for c in images], "all threshold images in one launch")
    # other thresholds move the same boxes to other kinds
    packed, out, loop = assert_outputs_equal([c[1] for c in images], [c[2] for c in images], "pos 0.55, bg 0.095", pos=.55, bg=.095)
    assert out.det_kind.tolist() == [LOC, LOC, BKG, LOC, LOC, LOC]


@pytest.fixture(scope="module")
def crowded():
    p, g = cases.crowded(np.random.default_rng(3), 257, 65)
    return p, g, cases.loop_errors([p], [g])


def test_past_the_thread_stride_and_the_wave_width(crowded):
    p, g, loop = crowded
    kind, fix = loop["det_kind"], loop["det_fix"]
    # a condition on the inputs, not a measurement
    assert set(kind.tolist()) == set(range(7)) and set(loop["gt_state"].tolist()) == set(range(4))
    assert set(fix[kind == LOC].tolist()) == {0, 1} and set(fix[kind == CLS].tolist()) == {0, 1}
    assert_outputs_equal([p], [g], "D = 257, G = 65, 3 classes", loop=loop)
    assert_outputs_equal([p], [g], "D = 257, G = 65 at pos 0.75, bg 0.3", pos=.75, bg=.3)


def test_lds_above_the_default_limit():
    """G = 1500 is 49 500 B of LDS: above the 48 KiB a launch gets without asking, below the 160 KiB of a CU"""
    p, g = cases.crowded(np.random.default_rng(4), 120, 1500, size=(2048, 1024))
    packed, out, loop = assert_outputs_equal([p], [g], "D = 120, G = 1500")
    assert {TP, IGNORED, LOC, BKG} <= set(out.det_kind.tolist()) and {DETECTED, DIFFICULT, MISSED} <= set(out.gt_state.tolist())


def test_workspace_fallback_next_to_an_lds_image():
    from da_detect_amd import _C

    rng = np.random.default_rng(5)
    small = cases.crowded(rng, 40, 9, size=(2048, 1024))
    big = cases.crowded(rng, 100, 5000, size=(2048, 1024))
    lds_only = _C.error_match_workspace_bytes([0, 40], [0, 9], 40, 9)
    assert _C.error_match_workspace_bytes([0, 40, 140], [0, 9, 5009], 140, 5009) >= lds_only + 33 * 5000
    packed, out, loop = assert_outputs_equal([small[0], big[0]], [small[1], big[1]], "G = 5000 in the workspace, G = 9 in LDS")
    kinds = out.det_kind.cpu().numpy()
    assert {TP, LOC} <= set(kinds[40:].tolist()) and TP in set(kinds[:40].tolist())
    # and the other way round: the workspace image first
    assert_outputs_equal([big[0], small[0]], [big[1], small[1]], "G = 5000 first")


def voc_flags_in_record_order(preds, gts, pos):
    """the existing matcher's flags at one threshold, brought from its (image, class, score) order into record order"""
    from da_detect_amd.data.evaluation.voc import voc_eval

    packed = voc_eval.pack(preds, gts)
    flags = voc_eval.match(packed, [pos])[0][0].cpu().numpy()
    score = np.concatenate([p.get_field("scores").numpy().astype(np.float32).astype(np.float64) for p in preds])
    label = np.concatenate([p.get_field("labels").numpy() for p in preds]).astype(np.int64)
    image = np.repeat(np.arange(len(preds)), [len(p) for p in preds])
    order = np.lexsort((-score, image * packed.n_class + label))                # data/evaluation/pairs.py pair_tables
    assert np.array_equal(packed.det_score, score[order]) and np.array_equal(packed.det_label, label[order])
    out = np.empty(len(order), dtype=np.int8)
    out[order] = flags
    return out


def test_tp_and_ignored_are_the_voc_matchers(crowded):
    edge = cases.edge_images()
    preds, gts = [crowded[0]] + [c[1] for c in edge], [crowded[1]] + [c[2] for c in edge]
    for pos in (.5, .75):
        packed, out = device_outputs(preds, gts, pos, .1)
        kind = out.det_kind.cpu().numpy()[packed.det_restore]
        voc = voc_flags_in_record_order(preds, gts, pos)
        assert np.array_equal(kind == TP, voc == 1) and np.array_equal(kind == IGNORED, voc == -1), pos
        assert (voc == 1).any() and (voc == -1).any() and (voc == 0).any()


@pytest.mark.parametrize("use_07", [False, True], ids=["area", "11-point"])
def test_ap_is_the_voc_scorers(use_07, tmp_path):
    """`ap` and `map` of summarise are eval_detection_voc's, equal as float64 values: the recorded VOC fixture and TWO_IMAGES"""
    from da_detect_amd.data.datasets import PascalVOCDataset
    from da_detect_amd.data.evaluation import errors
    from da_detect_amd.data.evaluation.voc import voc_eval

    dataset = PascalVOCDataset(write_voc_tree(tmp_path, TWO_IMAGES), "test", use_difficult=True)
    two = ([pred([[0, 0, 19, 29], [4, 5, 63, 47], [9, 11, 39, 43], [30, 1, 50, 20]], [7, 12, 15, 7], [.9, .8, .7, .6], (64, 48)),
            pred([[2, 3, 20, 25], [30, 30, 45, 38]], [2, 2], [.5, .4], (50, 40))], [dataset.get_groundtruth(0), dataset.get_groundtruth(1)])
    for what, (preds, gts) in (("fixture", fixture_boxlists(load_fixture())), ("TWO_IMAGES", two)):
        for pos in (.5, .75):
            want = voc_eval.eval_detection_voc(preds, gts, iou_thresh=pos, use_07_metric=use_07)
            packed, out, got = errors.analyse(preds, gts, pos, .1, use_07)
            assert got["ap"].dtype == np.float64 and np.array_equal(got["ap"], want["ap"], equal_nan=True), (what, pos, got["ap"], want["ap"])
            assert got["map"] == want["map"] and 0.0 < got["map"] <= 1.0 + AP_TOL, (what, pos)     # eleven times 1 / 11 is 1 + 2e-16
            loop = cases.loop_errors(preds, gts, pos, .1)
            assert_summary_close(got, cases.loop_summary(loop, packed.n_class, use_07), "%s at %.2f" % (what, pos))


def test_summarise_on_the_device_against_the_float64_loop(crowded):
    from da_detect_amd.data.evaluation import errors

    edge = cases.edge_images()
    preds, gts = [crowded[0]] + [c[1] for c in edge], [crowded[1]] + [c[2] for c in edge]
    loop = cases.loop_errors(preds, gts)
    for use_07 in (False, True):
        packed, out, got = errors.analyse(preds, gts, .5, .1, use_07)
        assert got["counts"].is_cuda and got["top_ranked"].is_cuda
        assert_summary_close(got, cases.loop_summary(loop, packed.n_class, use_07), "device, use_07_metric=%s" % use_07)


def test_malformed_input_is_refused_before_the_launch():
    from da_detect_amd import _C, _lib

    dev = torch.device("cuda")
    det = torch.tensor([[0., 0., 9., 9.], [0., 0., 9., 4.], [50., 50., 54., 54.]], device=dev)
    det_label = torch.tensor([1, 1, 2], dtype=torch.int32, device=dev)
    gt = torch.tensor([[0., 0., 9., 9.], [50., 50., 54., 54.]], device=dev)
    gt_label = torch.tensor([1, 1], dtype=torch.int32, device=dev)
    hard = torch.zeros(2, dtype=torch.uint8, device=dev)
    for det_off, gt_off in (([0, 2, 1], [0, 1, 2]), ([0, 2, 10 ** 6], [0, 1, 2]), ([0, 2, 3], [0, 5, 2]), ([1, 2, 3], [0, 1, 2]),
                            ([0, 2, 3], [0, 1, 1]), ([0, -1, 3], [0, 1, 2]), ([0, 2, 3], [0, 1])):
        with pytest.raises(_lib.DadetError) as err:
            _C.error_match(det, det_label, gt, gt_label, hard, det_off, gt_off)
        assert "status -1" in str(err.value) or "pairs + 1" in str(err.value)
    for pos, bg in ((.5, .5), (.5, 0.0), (1.01, .1), (.1, .5)):
        with pytest.raises(_lib.DadetError, match="status -1"):
            _C.error_match(det, det_label, gt, gt_label, hard, [0, 2, 3], [0, 1, 2], pos, bg)
    with pytest.raises(_lib.DadetError, match="int32"):
        _C.error_match(det, det_label.long(), gt, gt_label, hard, [0, 2, 3], [0, 1, 2])
    # nothing faulted: the well-formed call still runs, and gives the obvious answer — the exact box is the TP, the half box
    # (IoU 66 / 121) repeats it, and the box of image 2 sits exactly on a ground truth of another class
    kind, det_gt, same, other, fix, state, gt_det = _C.error_match(det, det_label, gt, gt_label, hard, [0, 2, 3], [0, 1, 2])
    torch.cuda.synchronize()
    assert kind.tolist() == [TP, cases.DUPE, CLS] and det_gt.tolist() == [0, 0, 1] and fix.tolist() == [0, 0, 1]
    assert state.tolist() == [DETECTED, COVERED] and gt_det.tolist() == [0, -1] and same.tolist()[0] == 1.0 and other.tolist()[2] == 1.0


# ------------------------------------------------------------------------------------------------ end to end
def _tiny_set(tmp_path):
    """TWO_IMAGES as a VOC tree and predictions for it (image 1 at twice its size): the car exactly, a person on the difficult
    box, a stray car, nothing on the dog (missed); image 2: a box far from the bicycle (missed)"""
    tree = write_voc_tree(tmp_path / "VOCtiny", TWO_IMAGES)
    predictions = [pred([[0, 0, 39, 59], [18, 22, 79, 87], [60, 2, 100, 40]], [7, 15, 7], [.9, .8, .75], (128, 96)),
                   pred([[30, 30, 45, 38]], [2], [.95], (50, 40))]
    saved = str(tmp_path / "predictions.pth")
    torch.save(predictions, saved)
    return tree, predictions, saved


def test_score_tool_writes_the_breakdown(tmp_path):
    from da_detect_amd.data.datasets import PascalVOCDataset

    tree, predictions, saved = _tiny_set(tmp_path)
    run = [sys.executable, os.path.join(ROOT, "tools", "score_net_da.py"), "--dataset", "voc:" + tree + ",test", "--predictions", saved,
           "--errors", "--bg-iou", "0.1", "--compare", saved]
    res = subprocess.run(run, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    dataset = PascalVOCDataset(tree, "test", use_difficult=True)
    preds = [p.resize((w, h)) for p, (_, w, h, _) in zip(predictions, TWO_IMAGES)]
    gts = [dataset.get_groundtruth(0), dataset.get_groundtruth(1)]
    loop = cases.loop_errors(preds, gts)
    assert loop["det_kind"].tolist() == [TP, IGNORED, cases.BOTH, BKG] and loop["gt_state"].tolist() == [DETECTED, DIFFICULT, MISSED, MISSED]
    want = cases.loop_summary(loop, 16, use_07_metric=True)
    got = json.load(open(str(tmp_path / "errors.json")))
    for key in ("counts", "missed", "covered", "n_pos", "confusion"):
        assert got[key] == want[key].tolist(), key
    nan_to = lambda values: np.array([np.nan if v is None else v for v in values], dtype=np.float64)      # noqa: E731
    assert_ap_close(nan_to(got["ap"]), want["ap"], "errors.json ap")
    assert_ap_close([got["map"]], [want["map"]], "errors.json map")
    for fix in cases.FIXES:
        assert_ap_close([got["dap"][fix]], [want["dap"][fix]], "errors.json dAP " + fix)
        assert_ap_close(nan_to(got["dap_by_class"][fix]), want["dap_by_class"][fix], "errors.json dAP %s per class" % fix)
    assert got["pos_thresh"] == .5 and got["bg_thresh"] == .1 and got["use_07_metric"] is True
    text = open(str(tmp_path / "errors.txt")).read()
    assert text in res.stderr and [line.split()[0] for line in text.splitlines()[2:]] == ["bicycle", "car", "dog", "person", "all"]
    assert "what changed" in res.stderr and os.path.exists(str(tmp_path / "result.txt"))


def test_draw_tool_colours_by_kind(tmp_path):
    from PIL import Image

    from da_detect_amd.data.evaluation import errors

    tree, predictions, saved = _tiny_set(tmp_path)
    tool = load_tool("draw_detections")
    common = ["--dataset", "voc:" + tree + ",test", "--predictions", saved, "--errors", "--gt"]
    host = tool.main(common + ["--out", str(tmp_path / "host"), "--host"])
    device = tool.main(common + ["--out", str(tmp_path / "device")])
    assert [os.path.basename(f) for f in host] == ["000001.png", "000002.png"] == [os.path.basename(f) for f in device]
    for a, b in zip(host, device):
        assert open(a, "rb").read() == open(b, "rb").read()
    plain = tool.main(["--dataset", "voc:" + tree + ",test", "--predictions", saved, "--gt", "--out", str(tmp_path / "plain"), "--host"])
    for path, plain_path, (_, w, h, _), kinds in zip(host, plain, TWO_IMAGES, ([TP, IGNORED, cases.BOTH], [BKG])):
        pixels = np.array(Image.open(path).convert("RGB"))
        assert pixels.shape == (2 * h, w, 3)
        panel = pixels[h:]                                                     # the predictions panel, under the ground truth
        has = lambda color: bool((panel == np.asarray(color, dtype=np.uint8)).all(-1).any())      # noqa: E731
        assert has(errors.MISSED_COLOR), "the missed ground truth is not drawn in %s" % path
        for k in kinds:                                                        # every detection is above the 0.7 of --threshold
            assert has(errors.KIND_COLORS[k]), (path, errors.KIND_NAMES[k])
        before = np.array(Image.open(plain_path).convert("RGB"))
        assert np.array_equal(before[:h], pixels[:h]) and not np.array_equal(before[h:], panel)      # the ground-truth panel stays
