"""Error breakdown of detections without a device: packing, the host-side checks of the launch, the ABI,
`summarise` on hand-made kernel outputs against closed forms and against the plain float64 loops of tests/_error_cases.py,
and the new flags of the two tools.

Tolerances.  Counts, states and the confusion table are integers: equal.  AP, dAP and the top-ranked shares are compared
with AP_TOL of tests/test_voc_eval.py (1e-9 absolute; the reasoning is stated there: sums of at most 1e6 float64 terms in
[0, 1] in a possibly different order)."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import _error_cases as cases
from _error_cases import BKG, BOTH, CLS, COVERED, DETECTED, DIFFICULT, DUPE, IGNORED, LOC, MISSED, TP
from test_voc_eval import ROOT, assert_ap_close, pred, truth


def load_tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def outputs_from(loop):
    """loop_errors' arrays (or hand-made ones) as the seven tensors of the launch, on the CPU"""
    from da_detect_amd.data.evaluation import errors

    return errors.Outputs(*(torch.from_numpy(np.ascontiguousarray(loop[k])) for k in errors.Outputs._fields))


def assert_summary_close(got, want, what):
    for key in ("counts", "missed", "covered", "n_pos", "confusion"):
        assert got[key].dtype == torch.int64 and np.array_equal(got[key].cpu().numpy(), want[key]), (what, key, got[key], want[key])
    assert_ap_close(got["ap"], want["ap"], what + ": ap")
    assert_ap_close([got["map"]], [want["map"]], what + ": map")
    for fix in cases.FIXES:
        assert_ap_close([got["dap"][fix]], [want["dap"][fix]], "%s: dAP %s" % (what, fix))
        assert_ap_close(got["dap_by_class"][fix], want["dap_by_class"][fix], "%s: dAP %s per class" % (what, fix))
    assert got["top_ranked"].dtype == torch.float64
    assert_ap_close(got["top_ranked"].cpu().numpy(), want["top_ranked"], what + ": top-ranked shares")


# ------------------------------------------------------------------------------------------------ pack
def test_pack_order_stability_and_round_trip():
    from da_detect_amd.data.evaluation import errors

    preds = [pred([[0, 0, 1, 1], [0, 0, 2, 2], [0, 0, 3, 3], [0, 0, 4, 4]], [2, 1, 2, 2], [.5, .25, .75, .5]),
             pred(np.zeros((0, 4)), [], []),
             pred([[0, 0, 5, 5], [0, 0, 6, 6]], [4, 1], [.125, .125])]
    gts = [truth([[0, 0, 9, 9], [1, 1, 8, 8]], [2, 4], [0, 1]), truth([[2, 2, 7, 7]], [1]), truth(np.zeros((0, 4)), [])]
    p = errors.pack(preds, gts)
    assert p.n_class == 5 and p.present.tolist() == [False, True, True, False, True]
    assert p.det_off.tolist() == [0, 4, 4, 6] and p.gt_off.tolist() == [0, 2, 3, 3]
    assert p.det_off.dtype == np.int32 and p.gt_off.dtype == np.int32
    # image, then descending score; the two .5 of image 0 and the two .125 of image 2 keep their record order
    assert p.det_box[:, 2].tolist() == [3.0, 1.0, 4.0, 2.0, 5.0, 6.0]
    assert p.det_score.tolist() == [.75, .5, .5, .25, .125, .125] and p.det_label.tolist() == [2, 2, 2, 1, 4, 1]
    assert p.det_order.tolist() == [2, 0, 3, 1, 4, 5] and p.det_restore.tolist() == [1, 3, 0, 2, 4, 5]
    records = np.concatenate([b.bbox.numpy() for b in preds])
    assert np.array_equal(p.det_box, records[p.det_order]) and np.array_equal(p.det_box[p.det_restore], records)
    assert p.gt_box[:, 0].tolist() == [0.0, 1.0, 2.0] and p.gt_label.tolist() == [2, 4, 1] and p.gt_difficult.tolist() == [0, 1, 0]
    assert p.det_box.dtype == np.float32 and p.gt_box.dtype == np.float32 and p.gt_difficult.dtype == np.uint8
    assert p.det_score.dtype == np.float64 and p.det_label.dtype == np.int64 and p.gt_label.dtype == np.int64
    empty = errors.pack([], [])
    assert empty.n_class == 0 and empty.det_off.tolist() == [0] and empty.gt_off.tolist() == [0]
    # the loop evaluator of the tests packs the same way
    loop = cases.loop_errors(preds, gts)
    assert loop["det_order"].tolist() == p.det_order.tolist() and loop["det_off"].tolist() == p.det_off.tolist()
    assert loop["det_label"].tolist() == p.det_label.tolist() and loop["gt_off"].tolist() == p.gt_off.tolist()


def test_pack_refusals():
    from da_detect_amd.data.evaluation import errors

    good_gt = truth([[0, 0, 1, 1]], [1])
    for bad in (pred([[0, 0, np.inf, 1]], [1], [.5]), pred([[0, 0, 1, 1]], [1], [np.nan]), pred([[np.nan, 0, 1, 1]], [1], [.5]),
                pred([[0, 0, 1, 1]], [1], [np.inf])):
        with pytest.raises(ValueError, match="non-finite"):
            errors.pack([bad], [good_gt])
    with pytest.raises(ValueError, match="non-finite"):
        errors.pack([pred([[0, 0, 1, 1]], [1], [.5])], [truth([[0, 0, -np.inf, 1]], [1])])
    with pytest.raises(ValueError, match="negative"):
        errors.pack([pred([[0, 0, 1, 1]], [-1], [.5])], [good_gt])
    with pytest.raises(ValueError, match="negative"):
        errors.pack([pred([[0, 0, 1, 1]], [1], [.5])], [truth([[0, 0, 1, 1]], [-2])])
    for box in ([5, 0, 4, 1], [0, 5, 1, 4]):
        with pytest.raises(ValueError, match="x2 < x1"):
            errors.pack([pred([box], [1], [.5])], [good_gt])
        with pytest.raises(ValueError, match="x2 < x1"):
            errors.pack([pred([[0, 0, 1, 1]], [1], [.5])], [truth([box], [1])])
    errors.pack([pred([[3, 3, 3, 3]], [1], [.5])], [good_gt])                    # a one-pixel box is a box
    with pytest.raises(AssertionError):
        errors.pack([], [good_gt])


def test_no_host_matcher_and_the_alias(monkeypatch):
    from da_detect_amd import _lib, compat
    from da_detect_amd.data.evaluation import errors

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_lib.DadetError, match="HIP device"):
        errors.analyse([pred([[0, 0, 1, 1]], [1], [.5])], [truth([[0, 0, 1, 1]], [1])])
    compat.install()
    import maskrcnn_benchmark.data.datasets.evaluation.errors as theirs

    assert theirs is errors
    assert len(errors.KIND_COLORS) == 7 and len(set(errors.KIND_COLORS + (errors.MISSED_COLOR,))) == 8
    assert (errors.TP, errors.IGNORED, errors.CLS, errors.LOC, errors.BOTH, errors.DUPE, errors.BKG) == (0, 1, 2, 3, 4, 5, 6)
    assert (errors.DETECTED, errors.DIFFICULT, errors.COVERED, errors.MISSED) == (0, 1, 2, 3)


# ------------------------------------------------------------------------------------------------ the launch, host side
def _launch_status(images, pos, bg):
    """dadet_error_match with no buffers at all: what it refuses before it looks at them"""
    from da_detect_amd import _C, _lib

    off, _ = _C._int_table([0] * (images + 1))
    _lib.call("dadet_error_match", None, None, None, None, None, off, off, images, 0, 0, ctypes.c_double(pos), ctypes.c_double(bg),
              None, ctypes.c_size_t(0), None, None, None, None, None, None, None, None)


def test_offset_tables_and_thresholds_are_checked_on_the_host():
    from da_detect_amd import _C, _lib

    assert _C.error_match_workspace_bytes([0, 3, 5], [0, 0, 2], 5, 2) > 0
    small = _C.error_match_workspace_bytes([0, 300], [0, 4900], 300, 4900)          # 33 * 4900 B fits the 160 KiB of LDS
    big = _C.error_match_workspace_bytes([0, 300], [0, 5000], 300, 5000)            # 33 * 5000 B does not
    assert small == _C.error_match_workspace_bytes([0, 300], [0, 9], 300, 9) and big >= small + 33 * 5000
    assert _C.error_match_workspace_bytes([0, 10 ** 6], [0, 1], 10 ** 6, 1) > 0      # detections of an image are not capped
    for det_off, gt_off, n_det, n_gt in (([1, 3], [0, 2], 3, 2),              # does not start at 0
                                         ([0, 3], [1, 2], 3, 2),
                                         ([0, 5, 3], [0, 1, 2], 3, 2),        # decreasing
                                         ([0, 2, 3], [0, 2, 1], 3, 1),
                                         ([0, -2, 3], [0, 1, 2], 3, 2),
                                         ([0, 3], [0, 9], 3, 2),              # runs past the array
                                         ([0, 10 ** 6, 3], [0, 0, 0], 3, 0),  # runs past the array in the middle
                                         ([0, 3], [0, 2], 4, 2)):             # ends short of the array
        with pytest.raises(_lib.DadetError, match="status -1"):
            _C.error_match_workspace_bytes(det_off, gt_off, n_det, n_gt)
    with pytest.raises(_lib.DadetError, match="pairs \\+ 1"):
        _C.error_match_workspace_bytes([0, 1, 2], [0, 1], 2, 1)
    # 0 < bg < pos <= 1, checked before any buffer is looked at
    for pos, bg in ((.5, .5), (.1, .5), (.5, 0.0), (.5, -.1), (1.5, .1), (float("nan"), .1), (.5, float("nan"))):
        with pytest.raises(_lib.DadetError, match="status -1"):
            _launch_status(1, pos, bg)
    _launch_status(0, .5, .1)                                                 # no images: nothing to do, and no error
    _launch_status(0, 1.0, .1)
    with pytest.raises(_lib.DadetError, match="status -1"):                   # well-ordered thresholds, but null buffers
        _launch_status(1, .5, .1)
    with pytest.raises(_lib.DadetError):                                      # no CPU path for the launch itself
        _C.error_match(torch.zeros(1, 4), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 4), torch.zeros(1, dtype=torch.int32),
                       torch.zeros(1, dtype=torch.uint8), [0, 1], [0, 1])


def test_error_match_abi():
    from da_detect_amd import _lib

    header = open(os.path.join(ROOT, "include", "dadet.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_args in (("dadet_error_match_workspace_bytes", 6), ("dadet_error_match", 22)):
        proto = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert proto, "include/dadet.h does not declare %s" % name
        assert len(proto.group(1).split(",")) == n_args
        assert len(_lib._SIGNATURES[name]) == n_args and name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name), "libdadet_hip.so does not export %s" % name
    order = re.search(r"\bint\s+dadet_error_match\s*\(([^;]*)\)\s*;", header).group(1)
    names = [re.split(r"[\s\*]+", part.strip())[-1] for part in order.split(",")]
    assert names == ["det_box", "det_label", "gt_box", "gt_label", "gt_difficult", "det_off_host", "gt_off_host", "images", "n_det",
                     "n_gt", "pos_thr", "bg_thr", "workspace", "workspace_bytes", "det_kind", "det_gt", "iou_same", "iou_other",
                     "det_fix", "gt_state", "gt_det", "stream"]


# ------------------------------------------------------------------------------------------------ the yardstick itself
def test_loop_evaluator_on_the_cases_with_known_answers():
    """the plain loop gives the kinds written next to each edge image, and the IoU values worked out by hand"""
    for what, p, g, kinds, fixes in cases.edge_images():
        loop = cases.loop_errors([p], [g])
        assert loop["det_kind"].tolist() == kinds and loop["det_fix"].tolist() == fixes, what
    loop = cases.loop_errors(*zip(*[(c[1], c[2]) for c in cases.edge_images()]))
    assert loop["det_kind"].tolist() == sum([c[3] for c in cases.edge_images()], [])
    for what, p, g, kind, iou in cases.threshold_images():
        loop = cases.loop_errors([p], [g])
        assert loop["det_kind"].tolist() == [kind], what
        got = loop["iou_same"][0]
        assert got.view(np.int32) == np.float32(iou).view(np.int32), (what, got, iou)
    assert np.float32(0.1) == np.float32(10) / np.float32(100) and float(np.float32(0.1)) >= 0.1
    none = cases.loop_errors([cases.edge_images()[1][1]], [cases.edge_images()[1][2]])
    assert none["det_gt"].tolist() == [-1, -1] and none["iou_same"].tolist() == [0.0, 0.0] and none["iou_other"].tolist() == [0.0, 0.0]


def crowded_loop():
    p, g = cases.crowded(np.random.default_rng(3), 257, 65)
    return p, g, cases.loop_errors([p], [g])


def test_crowded_generator_shows_every_value():
    """a condition on the inputs of the device test: all 7 kinds, all 4 states, and both fix values among Loc and among Cls"""
    p, g, loop = crowded_loop()
    kind, fix = loop["det_kind"], loop["det_fix"]
    print("kinds", np.bincount(kind, minlength=7).tolist(), "states", np.bincount(loop["gt_state"], minlength=4).tolist(),
          "fixes won", int(fix.sum()), "lost", int(((kind == LOC) | (kind == CLS)).sum() - fix.sum()))
    assert set(kind.tolist()) == {TP, IGNORED, CLS, LOC, BOTH, DUPE, BKG}
    assert set(loop["gt_state"].tolist()) == {DETECTED, DIFFICULT, COVERED, MISSED}
    assert set(fix[kind == LOC].tolist()) == {0, 1} and set(fix[kind == CLS].tolist()) == {0, 1}
    assert len(np.unique(loop["det_score"])) == 257 and set(loop["gt_label"].tolist()) == {1, 2, 3}
    # the row form of the IoU (used for the images with thousands of ground truths) is the scalar form, bit for bit
    rows = cases.loop_errors([p], [g], scalar_limit=0)
    for key in loop:
        assert np.array_equal(loop[key].view(np.int32) if loop[key].dtype == np.float32 else loop[key],
                              rows[key].view(np.int32) if rows[key].dtype == np.float32 else rows[key]), key


# ------------------------------------------------------------------------------------------------ summarise
def hand_made(preds, gts, det_kind, det_gt, det_fix, gt_state, gt_det):
    """(packed, outputs) with hand-made kernel outputs; the detections are given best first, so packed order = record order"""
    from da_detect_amd.data.evaluation import errors

    packed = errors.pack(preds, gts)
    assert packed.det_order.tolist() == list(range(len(det_kind)))
    n = len(det_kind)
    loop = dict(det_kind=np.array(det_kind, dtype=np.uint8), det_gt=np.array(det_gt, dtype=np.int32), iou_same=np.zeros(n, np.float32),
                iou_other=np.zeros(n, np.float32), det_fix=np.array(det_fix, dtype=np.uint8),
                gt_state=np.array(gt_state, dtype=np.uint8), gt_det=np.array(gt_det, dtype=np.int32), det_label=packed.det_label,
                det_score=packed.det_score, gt_label=packed.gt_label)
    return packed, outputs_from(loop), loop


def test_summarise_closed_form_one_class():
    """one class, ground truths A and B; d1 (.9) TP on A, d2 (.8) Loc on B with fix 1, d3 (.7) Bkg; area metric"""
    from da_detect_amd.data.evaluation import errors

    box = [0, 0, 9, 9]
    packed, outputs, loop = hand_made([pred([box] * 3, [1, 1, 1], [.9, .8, .7])], [truth([box] * 2, [1, 1])],
                                      [TP, LOC, BKG], [0, 1, -1], [0, 1, 0], [DETECTED, COVERED], [0, -1])
    got = errors.summarise(packed, outputs, use_07_metric=False)
    nan = float("nan")
    assert_ap_close(got["ap"], [nan, .5], "AP")
    assert_ap_close([got["map"]], [.5], "mAP")
    want = {"Loc": .5, "Bkg": 0.0, "Miss": 0.0, "FP": 0.0, "FN": .5, "Cls": 0.0, "Both": 0.0, "Dupe": 0.0}
    for fix, value in want.items():
        assert_ap_close([got["dap"][fix]], [value], "dAP " + fix)
        assert_ap_close(got["dap_by_class"][fix], [nan, value], "dAP %s per class" % fix)
    assert got["counts"].tolist() == [[0] * 7, [1, 0, 0, 1, 0, 0, 1]] and got["n_pos"].tolist() == [0, 2]
    assert got["missed"].tolist() == [0, 0] and got["covered"].tolist() == [0, 1]
    assert got["confusion"].tolist() == [[0, 0, 0], [0, 2, 1]]
    assert_ap_close(got["top_ranked"].numpy(), [[nan] * 3, [.5, .5, 0.0]], "top-ranked")     # the 2 best: one TP, one Loc
    assert_summary_close(got, cases.loop_summary(loop, 2, False), "one class")
    assert_summary_close(errors.summarise(packed, outputs, True), cases.loop_summary(loop, 2, True), "one class, 11-point")


def test_cls_fix_moves_a_detection_into_an_empty_class():
    """A (class 1) found by d1; d2 carries class 1 but sits on B (class 2), which has no detection of its own: fixing the
    classification gives class 2 its one true positive.  mAP (1 + 0) / 2 -> (1 + 1) / 2."""
    from da_detect_amd.data.evaluation import errors

    a, b = [0, 0, 9, 9], [20, 20, 29, 29]
    packed, outputs, loop = hand_made([pred([a, b], [1, 1], [.9, .8])], [truth([a, b], [1, 2])],
                                      [TP, CLS], [0, 1], [0, 1], [DETECTED, COVERED], [0, -1])
    nan = float("nan")
    for use_07 in (False, True):
        got = errors.summarise(packed, outputs, use_07)
        assert_ap_close(got["ap"], [nan, 1.0, 0.0], "AP")
        assert_ap_close([got["map"], got["dap"]["Cls"], got["dap"]["FN"], got["dap"]["Miss"]], [.5, .5, .5, 0.0], "mAP, dCls, dFN, dMiss")
        assert_ap_close(got["dap_by_class"]["Cls"], [nan, 0.0, 1.0], "dCls per class")
        assert got["confusion"].tolist() == [[0] * 4, [0, 1, 1, 0], [0] * 4] and got["covered"].tolist() == [0, 0, 1]
        assert_summary_close(got, cases.loop_summary(loop, 3, use_07), "moved detection")
    # without the fix claim the detection is only dropped
    packed, outputs, loop = hand_made([pred([a, b], [1, 1], [.9, .8])], [truth([a, b], [1, 2])],
                                      [TP, CLS], [0, 1], [0, 0], [DETECTED, COVERED], [0, -1])
    got = errors.summarise(packed, outputs)
    assert_ap_close([got["dap"]["Cls"]], [0.0], "dCls without the claim")
    assert_summary_close(got, cases.loop_summary(loop, 3, False), "dropped detection")


def test_a_fix_that_empties_a_class():
    """class 2 has one ground truth, missed: with the misses fixed it has no positives left and leaves the mean, as a class
    without positives does.  mAP (1 + 0) / 2 -> 1."""
    from da_detect_amd.data.evaluation import errors

    a, b = [0, 0, 9, 9], [20, 20, 29, 29]
    packed, outputs, loop = hand_made([pred([a], [1], [.9])], [truth([a, b], [1, 2])], [TP], [0], [0], [DETECTED, MISSED], [0, -1])
    nan = float("nan")
    got = errors.summarise(packed, outputs)
    assert got["missed"].tolist() == [0, 0, 1] and got["n_pos"].tolist() == [0, 1, 1]
    assert_ap_close(got["ap"], [nan, 1.0, 0.0], "AP")
    assert_ap_close([got["dap"]["Miss"], got["dap"]["FN"], got["dap"]["FP"]], [.5, .5, 0.0], "dMiss, dFN, dFP")
    assert_ap_close(got["dap_by_class"]["Miss"], [nan, 0.0, nan], "dMiss per class")
    assert_summary_close(got, cases.loop_summary(loop, 3, False), "emptied class")


@pytest.mark.parametrize("use_07", [False, True], ids=["area", "11-point"])
def test_summarise_against_the_float64_loop(use_07):
    """the loop evaluator's outputs for the 257 / 65 image and the edge images, fed to summarise on the CPU"""
    from da_detect_amd.data.evaluation import errors

    p, g = cases.crowded(np.random.default_rng(3), 257, 65)
    edge = cases.edge_images()
    preds, gts = [p] + [c[1] for c in edge], [g] + [c[2] for c in edge]
    loop = cases.loop_errors(preds, gts)
    packed = errors.pack(preds, gts)
    assert packed.det_order.tolist() == loop["det_order"].tolist()
    got = errors.summarise(packed, outputs_from(loop), use_07)
    want = cases.loop_summary(loop, packed.n_class, use_07)
    assert_summary_close(got, want, "crowded and edge images")
    assert 0.0 < got["map"] < 1.0 and got["dap"]["FP"] > 0 and got["dap"]["FN"] > 0
    assert int(got["counts"].sum()) == len(loop["det_kind"]) and int(got["confusion"].sum()) == int((loop["det_kind"] != IGNORED).sum())
    text = errors.table(got, lambda k: "class%d" % k)
    assert text.splitlines()[0].split() == ["class"] + list(errors._COLUMNS) and text.splitlines()[-1].startswith("all")
    assert len(text.splitlines()) == 1 + 3 + 1


# ------------------------------------------------------------------------------------------------ tools
def test_tools_accept_the_new_flags():
    score = load_tool("score_net_da").build_parser()
    args = score.parse_args(["--dataset", "ann.json,imgs", "--predictions", "p.pth", "--errors", "--bg-iou", "0.2", "--compare", "q.pth"])
    assert args.errors and args.bg_iou == 0.2 and args.compare == "q.pth"
    args = score.parse_args(["--dataset", "voc:/d/VOC2007,test", "--predictions", "p.pth"])
    assert not args.errors and args.bg_iou == 0.1 and args.compare is None
    draw = load_tool("draw_detections").build_parser()
    args = draw.parse_args(["--dataset", "ann.json,imgs", "--predictions", "p.pth", "--out", "figs", "--errors", "--host"])
    assert args.errors and args.host and args.bg_iou == 0.1 and args.errors_iou == 0.5
    assert not draw.parse_args(["--dataset", "ann.json,imgs", "--predictions", "p.pth", "--out", "figs"]).errors
