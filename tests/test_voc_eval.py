"""PASCAL VOC AP without a device: packing, accumulation and both AP metrics against the reference's recorded curves, the VOC
dataset, catalog, builder, dispatch, aliases, and the host-side checks of the match launch.  tests/test_voc_eval_gpu.py
imports the plain evaluator and the fixture helpers below.

Yardsticks.
  * tests/golden/voc_eval_cases.npz (tests/golden/make_golden_voc_eval.py): the REFERENCE's `calc_detection_voc_prec_rec` /
    `calc_detection_voc_ap` on a seeded set with distinct scores, at IoU 0.5 and 0.75, both metrics.
  * `loop_voc`: a plain evaluator of the same rule, one Python loop per pair, IoU from this package's torch float32
    `boxlist_iou` on the CPU (which states the reference's operations one for one; the fixture pins the two together end
    to end on the device).

Tolerances.  `prec` and `rec` are the same float64 operations as the reference's (an integer cumsum, one division): equal
with np.array_equal where not nan, and nan in the same places.  AP is a sum of at most L <= 1e6 float64 terms in [0, 1]
whose order of summation may differ from numpy's pairwise sum: L * 2^-53 ~ 1e-10, so 1e-9 absolute leaves a decade.

The fixture stores curves, not match flags.  `flags_from_curves` recovers flags that reproduce a curve: tp = rec * n_pos and
fp = tp / prec - tp, rounded (both are small integers), give a 1 where tp steps and a 0 where fp steps, -1 elsewhere.  While
tp is still 0 the precision is nan (nothing counted yet) or 0 (some false positive counted) and the number of false
positives is not recorded; any split that reaches the next known count gives the same curve, and the helper takes the
leftmost one.  A class without positives has no `rec`: its tp is 0 throughout."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
AP_TOL = 1e-9
SIZE = (640, 480)


# ------------------------------------------------------------------------------------------------ shared helpers
def boxlist(boxes, size=SIZE, **fields):
    from da_detect_amd.structures.bounding_box import BoxList

    out = BoxList(torch.as_tensor(np.asarray(boxes, dtype=np.float32)).reshape(-1, 4), size, mode="xyxy")
    for name, values in fields.items():
        out.add_field(name, torch.as_tensor(np.asarray(values)))
    return out


def pred(boxes, labels, scores, size=SIZE):
    return boxlist(boxes, size, labels=np.asarray(labels, dtype=np.int64), scores=np.asarray(scores, dtype=np.float32))


def truth(boxes, labels, difficult=None, size=SIZE):
    difficult = np.zeros(len(labels), dtype=np.uint8) if difficult is None else np.asarray(difficult, dtype=np.uint8)
    return boxlist(boxes, size, labels=np.asarray(labels, dtype=np.int64), difficult=difficult)


def load_fixture():
    return dict(np.load(os.path.join(HERE, "golden", "voc_eval_cases.npz")))


def fixture_boxlists(fx):
    preds, gts = [], []
    for i, (w, h) in enumerate(fx["image_size"].tolist()):
        d, g = fx["det_image"] == i, fx["gt_image"] == i
        preds.append(pred(fx["det_box"][d], fx["det_label"][d], fx["det_score"][d], (w, h)))
        gts.append(truth(fx["gt_box"][g], fx["gt_label"][g], fx["gt_difficult"][g], (w, h)))
    return preds, gts


def fixture_curves(fx, t):
    """the reference's (prec, rec) lists at threshold index t, None holes restored"""
    out = []
    for name in ("prec", "rec"):
        flat, off, present = fx["%s_%d" % (name, t)], fx["%s_off_%d" % (name, t)], fx["%s_present_%d" % (name, t)]
        out.append([flat[off[k]:off[k + 1]] if present[k] else None for k in range(len(present))])
    return out


def assert_curves_equal(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), "%s: label %d is %s here, %s in the yardstick" % (what, k, type(g), type(w))
        if w is None:
            continue
        assert g.dtype == np.float64 and g.shape == w.shape, (what, k, g.shape, w.shape)
        assert np.array_equal(np.isnan(g), np.isnan(w)), "%s: label %d has nan elsewhere" % (what, k)
        ok = ~np.isnan(w)
        assert np.array_equal(g[ok], w[ok]), "%s: label %d differs first at %s" % (what, k, np.flatnonzero(g[ok] != w[ok])[:3])


def assert_ap_close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: nan at %s, yardstick %s" % (what, np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok]).max() if ok.any() else 0.0
    print("%s: largest AP difference %.3e (tolerance %.0e)" % (what, err, AP_TOL))
    assert err <= AP_TOL, (what, got, want)


def loop_voc(pred_boxlists, gt_boxlists, thresholds):
    """The rule, plainly.  -> dict: `match` int8 [T, Nd], `gt_index` int32 [Nd], `iou_max` float32 [Nd], `n_pos` [P] — all in
    packed order (images ascending, labels ascending, score descending with ties in record order) — and per threshold the
    reference-shaped `prec` / `rec` lists (ties between equal scores: image order, then the pair's order)."""
    from da_detect_amd.structures.boxlist_ops import boxlist_iou

    T = len(thresholds)
    match, gt_index, iou_max, n_pos, labels_of, scores_of = [[] for _ in range(T)], [], [], [], [], []
    seen = set()
    for p, g in zip(pred_boxlists, gt_boxlists):
        pl, ps = p.get_field("labels").numpy(), p.get_field("scores").numpy()
        gl, gd = g.get_field("labels").numpy(), g.get_field("difficult").numpy().astype(bool)
        for label in np.unique(np.concatenate([pl, gl]).astype(int)):
            seen.add(int(label))
            order = np.flatnonzero(pl == label)
            order = order[np.argsort(-ps[order].astype(np.float64), kind="stable")]
            boxes = p.bbox[torch.from_numpy(order)].clone()
            gts, hard = g.bbox[torch.from_numpy(np.flatnonzero(gl == label))].clone(), gd[gl == label]
            n_pos.append(int((~hard).sum()))
            labels_of.extend([int(label)] * len(order))
            scores_of.extend(ps[order].tolist())
            if len(order) == 0:
                continue
            if len(gts) == 0:
                gt_index.extend([-1] * len(order))
                iou_max.extend([0.0] * len(order))
                for t in range(T):
                    match[t].extend([0] * len(order))
                continue
            boxes[:, 2:] += 1
            gts[:, 2:] += 1
            iou = boxlist_iou(boxlist(boxes, g.size), boxlist(gts, g.size)).numpy()
            assert iou.dtype == np.float32
            best = iou.argmax(axis=1)
            gt_index.extend(best.tolist())
            iou_max.extend(iou.max(axis=1).tolist())
            for t, thr in enumerate(thresholds):
                cut = best.copy()
                cut[iou.max(axis=1) < thr] = -1
                taken = np.zeros(len(gts), dtype=bool)
                for c in cut:
                    if c < 0:
                        match[t].append(0)
                        continue
                    match[t].append(-1 if hard[c] else (0 if taken[c] else 1))
                    taken[c] = True
    out = {"match": np.array(match, dtype=np.int8).reshape(T, -1), "gt_index": np.array(gt_index, dtype=np.int32),
           "iou_max": np.array(iou_max, dtype=np.float32), "n_pos": np.array(n_pos, dtype=np.int32), "prec": [], "rec": []}
    K = max(seen) + 1 if seen else 0
    labels_of, scores_of = np.array(labels_of, dtype=np.int64), np.array(scores_of, dtype=np.float64)
    pair_label = []
    for p, g in zip(pred_boxlists, gt_boxlists):
        pair_label.extend(np.unique(np.concatenate([p.get_field("labels").numpy(), g.get_field("labels").numpy()])).tolist())
    pair_label = np.array(pair_label, dtype=np.int64)
    for t in range(T):
        prec, rec = [None] * K, [None] * K
        for k in sorted(seen):
            mine = np.flatnonzero(labels_of == k)
            m = out["match"][t][mine[np.argsort(-scores_of[mine], kind="stable")]]
            tp, fp = np.cumsum(m == 1), np.cumsum(m == 0)
            with np.errstate(invalid="ignore", divide="ignore"):
                prec[k] = tp / (fp + tp)
                total = int(out["n_pos"][pair_label == k].sum())
                if total > 0:
                    rec[k] = tp / total
        out["prec"].append(prec)
        out["rec"].append(rec)
    return out


def loop_ap(prec, rec, use_07_metric):
    """the two PASCAL VOC metrics, per class, in plain numpy"""
    ap = np.full(len(prec), np.nan)
    for k in range(len(prec)):
        if prec[k] is None or rec[k] is None:
            continue
        p, r = np.nan_to_num(prec[k]), rec[k]
        if use_07_metric:
            ap[k] = 0.0
            for t in np.arange(0.0, 1.1, 0.1):
                ap[k] += (p[r >= t].max() if (r >= t).any() else 0.0) / 11
        else:
            mpre, mrec = np.concatenate(([0.0], p, [0.0])), np.concatenate(([0.0], r, [1.0]))
            mpre = np.maximum.accumulate(mpre[::-1])[::-1]
            i = np.flatnonzero(mrec[1:] != mrec[:-1])
            ap[k] = np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])
    return ap


def flags_from_curves(prec, rec, n_pos):
    """match flags of one class, in descending score, that reproduce its recorded curve (module docstring)"""
    n = len(prec)
    tp = np.zeros(n, dtype=np.int64) if rec is None else np.rint(rec * n_pos).astype(np.int64)
    fp = np.full(n, -1, dtype=np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        known = tp > 0
        fp[known] = np.rint(tp[known] / prec[known] - tp[known]).astype(np.int64)
    fp[(tp == 0) & np.isnan(prec)] = 0
    unknown = np.flatnonzero(fp < 0)                     # tp == 0 and prec == 0: one run, at least one false positive
    if len(unknown):
        s, e = unknown[0], unknown[-1]
        assert np.array_equal(unknown, np.arange(s, e + 1))
        # the element after the run is the first true positive, so the run ends at that element's count
        target = fp[e + 1] if e + 1 < n else e - s + 1
        fp[s:e + 1] = np.minimum(np.arange(1, e - s + 2), target)
    d_tp, d_fp = np.diff(np.concatenate(([0], tp))), np.diff(np.concatenate(([0], fp)))
    assert ((d_tp >= 0) & (d_fp >= 0) & (d_tp + d_fp <= 1)).all()
    return np.where(d_tp == 1, 1, np.where(d_fp == 1, 0, -1)).astype(np.int8)


def write_voc_tree(root, images, split="test"):
    """images: list of (id, width, height, [(name, xmin, ymin, xmax, ymax, difficult), ...]) -> a VOC-layout tree under root"""
    from PIL import Image

    for sub in ("Annotations", "JPEGImages", os.path.join("ImageSets", "Main")):
        os.makedirs(os.path.join(str(root), sub), exist_ok=True)
    for name, w, h, objects in images:
        body = "".join("<object><name>%s</name><difficult>%d</difficult><bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax>"
                       "<ymax>%d</ymax></bndbox></object>" % (o[0], o[5], o[1], o[2], o[3], o[4]) for o in objects)
        with open(os.path.join(str(root), "Annotations", name + ".xml"), "w") as f:
            f.write("<annotation><filename>%s.jpg</filename><size><width>%d</width><height>%d</height><depth>3</depth></size>%s"
                    "</annotation>" % (name, w, h, body))
        Image.fromarray(np.full((h, w, 3), 90, dtype=np.uint8)).save(os.path.join(str(root), "JPEGImages", name + ".jpg"))
    with open(os.path.join(str(root), "ImageSets", "Main", split + ".txt"), "w") as f:
        f.write("".join(name + "\n" for name, _, _, _ in images))
    return str(root)


TWO_IMAGES = [("000001", 64, 48, [("car", 1, 1, 20, 30, 0), ("person", 10, 12, 40, 44, 1), ("Dog ", 5, 6, 64, 48, 0)]),
              ("000002", 50, 40, [("bicycle", 3, 4, 25, 26, 0)])]


# ------------------------------------------------------------------------------------------------ scorer, host side
def test_pack_offsets_and_order():
    from da_detect_amd.data.evaluation.voc import voc_eval

    preds = [pred([[0, 0, 1, 1], [0, 0, 2, 2], [0, 0, 3, 3], [0, 0, 4, 4]], [2, 1, 2, 2], [.5, .25, .75, .5]),
             pred(np.zeros((0, 4)), [], []),
             pred([[0, 0, 5, 5]], [4], [.125])]
    gts = [truth([[0, 0, 9, 9], [1, 1, 8, 8]], [2, 4], [0, 1]), truth([[2, 2, 7, 7]], [1]), truth(np.zeros((0, 4)), [])]
    p = voc_eval.pack(preds, gts)
    K = 5
    assert p.n_class == K and p.present.tolist() == [False, True, True, False, True]
    assert p.pair_key.tolist() == [0 * K + 1, 0 * K + 2, 0 * K + 4, 1 * K + 1, 2 * K + 4]
    assert p.det_off.tolist() == [0, 1, 4, 4, 4, 5] and p.gt_off.tolist() == [0, 0, 1, 2, 3, 3]
    assert p.det_off.dtype == np.int32 and p.gt_off.dtype == np.int32
    assert p.det_box[:, 2].tolist() == [2.0, 3.0, 1.0, 4.0, 5.0]          # pair, then score descending, ties in record order
    assert p.det_score.tolist() == [.25, .75, .5, .5, .125] and p.det_label.tolist() == [1, 2, 2, 2, 4]
    assert p.det_box.dtype == np.float32 and p.gt_box.dtype == np.float32 and p.gt_difficult.dtype == np.uint8
    assert p.gt_box[:, 0].tolist() == [0.0, 1.0, 2.0] and p.gt_difficult.tolist() == [0, 1, 0]
    for bad in (pred([[0, 0, np.inf, 1]], [1], [.5]), pred([[0, 0, 1, 1]], [1], [np.nan]), pred([[np.nan, 0, 1, 1]], [1], [.5])):
        with pytest.raises(ValueError, match="non-finite"):
            voc_eval.pack([bad], [truth([[0, 0, 1, 1]], [1])])
    with pytest.raises(ValueError, match="non-finite"):
        voc_eval.pack([pred([[0, 0, 1, 1]], [1], [.5])], [truth([[0, 0, -np.inf, 1]], [1])])
    empty = voc_eval.pack([], [])
    assert empty.n_class == 0 and empty.det_off.tolist() == [0] and len(empty.pair_key) == 0


@pytest.fixture(scope="module")
def fixture():
    return load_fixture()


def _fixture_flags(fx, packed, t):
    """the recovered flags of every class, brought into packed order"""
    prec, rec = fixture_curves(fx, t)
    flags = np.full(len(packed.det_score), 9, dtype=np.int8)
    for k in range(len(prec)):
        if prec[k] is None:
            continue
        mine = np.flatnonzero(packed.det_label == k)
        mine = mine[np.argsort(-packed.det_score[mine], kind="stable")]
        flags[mine] = flags_from_curves(prec[k], rec[k], int(fx["n_pos"][k]))
    assert (flags != 9).all()
    return flags


def test_accumulate_and_ap_reproduce_the_reference_curves(fixture):
    from da_detect_amd.data.evaluation.voc import voc_eval

    fx = fixture
    assert len(np.unique(fx["det_score"])) == len(fx["det_score"])       # distinct: no tie order to speak of
    packed = voc_eval.pack(*fixture_boxlists(fx))
    assert packed.n_class == 7 and packed.present.tolist() == [False, True, True, True, False, True, True]
    T = len(fx["thresholds"])
    flags = torch.from_numpy(np.stack([_fixture_flags(fx, packed, t) for t in range(T)]))
    assert (flags[0] != flags[1]).any()
    hard = packed.gt_difficult.astype(np.int64)
    n_pos = torch.tensor([int((1 - hard[a:b]).sum()) for a, b in zip(packed.gt_off[:-1], packed.gt_off[1:])], dtype=torch.int32)
    curves = voc_eval.accumulate(packed, flags, n_pos)
    assert curves.n_pos.tolist() == fx["n_pos"].tolist() and curves.prec.dtype == torch.float64
    for t in range(T):
        want_prec, want_rec = fixture_curves(fx, t)
        got_prec, got_rec = voc_eval._curve_lists(curves, t)
        assert_curves_equal(got_prec, want_prec, "prec at IoU %.2f" % fx["thresholds"][t])
        assert_curves_equal(got_rec, want_rec, "rec at IoU %.2f" % fx["thresholds"][t])
        for m, use_07 in enumerate((True, False)):
            what = "IoU %.2f %s" % (fx["thresholds"][t], "11-point" if use_07 else "area")
            # the reference's signature, fed the reference's own curves ...
            assert_ap_close(voc_eval.calc_detection_voc_ap(want_prec, want_rec, use_07_metric=use_07), fx["ap"][t, m], what)
            assert_ap_close(loop_ap(want_prec, want_rec, use_07), fx["ap"][t, m], what + " (the test's own)")
    # ... and the batched form over all thresholds at once
    for m, use_07 in enumerate((True, False)):
        ap = voc_eval.average_precision(curves.prec, curves.rec, curves.count, use_07).numpy()
        ap[:, ~(curves.present & (curves.n_pos > 0))] = np.nan
        assert_ap_close(ap, fx["ap"][:, m], "batched, use_07_metric=%s" % use_07)
        for t in range(T):
            assert abs(voc_eval._nanmean(ap[t]) - fx["map"][t, m]) <= AP_TOL


def test_plain_evaluator_matches_the_reference_curves(fixture):
    """the yardstick of the device tests, itself held to the reference: with this package's float32 boxlist_iou on the CPU the
    plain loop gives the recorded curves exactly, so that IoU equals the reference's wherever it decides a flag"""
    preds, gts = fixture_boxlists(fixture)
    loop = loop_voc(preds, gts, fixture["thresholds"].tolist())
    for t in range(len(fixture["thresholds"])):
        want_prec, want_rec = fixture_curves(fixture, t)
        assert_curves_equal(loop["prec"][t], want_prec, "loop prec")
        assert_curves_equal(loop["rec"][t], want_rec, "loop rec")
    assert (loop["match"] == -1).any() and (loop["match"][0] != loop["match"][1]).any()


def test_ap_functions_on_hand_cases():
    from da_detect_amd.data.evaluation.voc.voc_eval import calc_detection_voc_ap

    nan = float("nan")
    prec = [None, np.array([1.0, .5, 2 / 3, .5]), np.array([nan, nan, 0.0]), np.zeros(0), np.array([nan, 1.0])]
    rec = [None, np.array([.5, .5, 1.0, 1.0]), None, np.zeros(0), np.array([0.0, 1.0])]
    area = calc_detection_voc_ap(prec, rec, use_07_metric=False)
    assert_ap_close(area, [nan, .5 * 1.0 + .5 * (2 / 3), nan, 0.0, 1.0], "area, by hand")
    eleven = calc_detection_voc_ap(prec, rec, use_07_metric=True)
    assert_ap_close(eleven, [nan, (6 * 1.0 + 5 * (2 / 3)) / 11, nan, 0.0, 1.0], "11-point, by hand")
    assert_ap_close(area, loop_ap(prec, rec, False), "area, plain numpy")
    assert_ap_close(eleven, loop_ap(prec, rec, True), "11-point, plain numpy")
    assert calc_detection_voc_ap([], [], use_07_metric=True).shape == (0,)


def test_no_host_matcher(monkeypatch):
    from da_detect_amd import _lib
    from da_detect_amd.data.evaluation.voc import voc_eval

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_lib.DadetError, match="HIP device"):
        voc_eval.eval_detection_voc([pred([[0, 0, 1, 1]], [1], [.5])], [truth([[0, 0, 1, 1]], [1])])


# ------------------------------------------------------------------------------------------------ the launch, host side
def test_offset_tables_are_checked_on_the_host():
    """the workspace query runs the launch's own checks and needs no device: a malformed table is an error return"""
    from da_detect_amd import _C, _lib

    assert _C.voc_match_workspace_bytes([0, 3, 5], [0, 0, 2], 5, 2, 2) > 0
    small = _C.voc_match_workspace_bytes([0, 300], [0, 2000], 300, 2000, 16)       # 81 * 2000 B fits the 160 KiB of LDS
    big = _C.voc_match_workspace_bytes([0, 300], [0, 2100], 300, 2100, 16)         # 81 * 2100 B does not
    assert big >= small + 81 * 2100
    assert _C.voc_match_workspace_bytes([0, 10 ** 6], [0, 1], 10 ** 6, 1, 1) > 0   # detections of a pair are not capped
    for det_off, gt_off, n_det, n_gt in (([1, 3], [0, 2], 3, 2),              # does not start at 0
                                         ([0, 3], [1, 2], 3, 2),
                                         ([0, 5, 3], [0, 1, 2], 3, 2),        # decreasing
                                         ([0, 2, 3], [0, 2, 1], 3, 1),
                                         ([0, -2, 3], [0, 1, 2], 3, 2),
                                         ([0, 3], [0, 9], 3, 2),              # runs past the array
                                         ([0, 10 ** 6, 3], [0, 0, 0], 3, 0),  # runs past the array in the middle
                                         ([0, 3], [0, 2], 4, 2)):             # ends short of the array
        with pytest.raises(_lib.DadetError, match="status -1"):
            _C.voc_match_workspace_bytes(det_off, gt_off, n_det, n_gt, 2)
    for n_thr in (0, 17, -1):
        with pytest.raises(_lib.DadetError, match="status -1"):
            _C.voc_match_workspace_bytes([0, 1], [0, 1], 1, 1, n_thr)
    assert _C.voc_match_workspace_bytes([0, 1], [0, 1], 1, 1, 1) > 0 and _C.voc_match_workspace_bytes([0, 1], [0, 1], 1, 1, 16) > 0
    with pytest.raises(_lib.DadetError, match="pairs \\+ 1"):
        _C.voc_match_workspace_bytes([0, 1, 2], [0, 1], 2, 1, 1)
    with pytest.raises(_lib.DadetError):                                     # no CPU path for the launch itself
        _C.voc_match(torch.zeros(1, 4), torch.zeros(1, 4), torch.zeros(1, dtype=torch.uint8), [0, 1], [0, 1], [.5])


def test_voc_match_abi():
    from da_detect_amd import _lib

    header = open(os.path.join(ROOT, "include", "dadet.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_args in (("dadet_voc_match_workspace_bytes", 7), ("dadet_voc_match", 17)):
        proto = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert proto, "include/dadet.h does not declare %s" % name
        assert len(proto.group(1).split(",")) == n_args
        assert len(_lib._SIGNATURES[name]) == n_args and name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name), "libdadet_hip.so does not export %s" % name


# ------------------------------------------------------------------------------------------------ datasets
def test_pascal_voc_dataset(tmp_path):
    from da_detect_amd.data.datasets import PascalVOCDataset

    root = write_voc_tree(tmp_path, TWO_IMAGES)
    kept = PascalVOCDataset(root, "test", use_difficult=True)
    assert len(kept) == 2 and kept.ids == ["000001", "000002"] and kept.id_to_img_map == {0: "000001", 1: "000002"}
    assert len(PascalVOCDataset.CLASSES) == 21 and kept.map_class_id_to_class_name(7) == "car"
    gt = kept.get_groundtruth(0)
    assert gt.mode == "xyxy" and gt.size == (64, 48)
    assert gt.bbox.tolist() == [[0., 0., 19., 29.], [9., 11., 39., 43.], [4., 5., 63., 47.]] and gt.bbox.dtype == torch.float32
    assert gt.get_field("labels").tolist() == [7, 15, 12] and gt.get_field("difficult").tolist() == [False, True, False]
    assert kept.get_img_info(0) == {"height": 48, "width": 64} and kept.get_img_info(1) == {"height": 40, "width": 50}

    dropped = PascalVOCDataset(root, "test", is_source=False)
    gt = dropped.get_groundtruth(0)
    assert gt.get_field("labels").tolist() == [7, 12] and gt.get_field("difficult").tolist() == [False, False]
    img, target, index = dropped[0]
    assert index == 0 and img.size == (64, 48) and target.get_field("is_source").tolist() == [False, False]
    assert kept[1][1].get_field("is_source").tolist() == [True] and kept[1][1].get_field("labels").tolist() == [2]
    tensor, target, _ = PascalVOCDataset(root, "test", decode_to_tensor=True)[1]
    assert tensor.dtype == torch.uint8 and tuple(tensor.shape) == (40, 50, 3) and len(target) == 1
    seen = []
    with_tf = PascalVOCDataset(root, "test", transforms=lambda im, t: (seen.append(im.size) or "img", t))
    assert with_tf[1][0] == "img" and seen == [(50, 40)]

    own = PascalVOCDataset(root, "test", use_difficult=True, classes=("__background__", "person", "dog", "bicycle", "car"))
    assert own.get_groundtruth(0).get_field("labels").tolist() == [4, 1, 2] and own.map_class_id_to_class_name(3) == "bicycle"
    assert len(PascalVOCDataset.CLASSES) == 21                                  # the override is the instance's own
    none = write_voc_tree(tmp_path / "bare", [("a", 10, 8, [])])
    gt = PascalVOCDataset(none, "test").get_groundtruth(0)
    assert tuple(gt.bbox.shape) == (0, 4) and len(PascalVOCDataset(none, "test")[0][1]) == 0


def test_coco_dataset_groundtruth_for_voc_scoring(tmp_path):
    import json

    from da_detect_amd.data.datasets import COCODataset

    path = os.path.join(str(tmp_path), "ann.json")
    with open(path, "w") as f:
        json.dump({"images": [{"id": 5, "file_name": "a.png", "width": 100, "height": 80}],
                   "annotations": [{"id": 1, "image_id": 5, "category_id": 26, "bbox": [10, 20, 30, 40], "area": 1200, "iscrowd": 0},
                                   {"id": 2, "image_id": 5, "category_id": 24, "bbox": [0, 0, 50, 50], "area": 2500, "iscrowd": 1}],
                   "categories": [{"id": 24, "name": "person"}, {"id": 26, "name": "car"}]}, f)
    ds = COCODataset(path, str(tmp_path), remove_images_without_annotations=False)
    gt = ds.get_groundtruth(0)
    assert gt.mode == "xyxy" and gt.size == (100, 80) and gt.bbox.tolist() == [[10., 20., 39., 59.], [0., 0., 49., 49.]]
    assert gt.get_field("labels").tolist() == [2, 1] and gt.get_field("difficult").tolist() == [False, True]
    assert [ds.map_class_id_to_class_name(i) for i in (1, 2)] == ["person", "car"]


def test_catalog_names_and_register_voc(monkeypatch):
    from da_detect_amd.config.paths_catalog import DatasetCatalog

    monkeypatch.setenv("DADET_DATA_DIR", "/data")
    for year in ("2007", "2012"):
        for split in ("train", "val", "test"):
            got = DatasetCatalog.get("voc_%s_%s" % (year, split))
            assert got == {"factory": "PascalVOCDataset", "args": {"data_dir": "/data/voc/VOC%s" % year, "split": split}}
    assert DatasetCatalog.get("cityscapes_fine_instanceonly_seg_val_cocostyle")["factory"] == "COCODataset"
    with pytest.raises(RuntimeError, match="Dataset not available"):
        DatasetCatalog.get("voc_2030_test")
    monkeypatch.setattr(DatasetCatalog, "DATASETS", dict(DatasetCatalog.DATASETS))
    DatasetCatalog.register_voc("cityscapes_voc_val", "/abs/cityscapes_voc", "val")
    assert DatasetCatalog.get("cityscapes_voc_val") == {"factory": "PascalVOCDataset",
                                                        "args": {"data_dir": "/abs/cityscapes_voc", "split": "val"}}
    DatasetCatalog.register("voc_as_cocostyle", "img", "ann.json")             # "coco" in the name still wins
    assert DatasetCatalog.get("voc_as_cocostyle")["factory"] == "COCODataset"
    for bad in ("clipart_test", "voc_cocostyle"):
        with pytest.raises(ValueError):
            DatasetCatalog.register_voc(bad, "x", "test")


def test_from_catalog_sets_use_difficult(tmp_path):
    from da_detect_amd.data import build
    from da_detect_amd.data.datasets import PascalVOCDataset, TripletDataset

    root = write_voc_tree(tmp_path, TWO_IMAGES, split="trainval")

    class Catalog(object):
        @staticmethod
        def get(name):
            return dict(factory="PascalVOCDataset", args=dict(data_dir=root, split="trainval"))

    train = build._from_catalog("voc_x", Catalog, None, True, False)
    test = build._from_catalog("voc_x", Catalog, None, False, True)
    assert isinstance(train, PascalVOCDataset) and train.keep_difficult is False and train.is_source is False
    assert test.keep_difficult is True and test.is_source is True
    assert len(train.get_groundtruth(0)) == 2 and len(test.get_groundtruth(0)) == 3
    # VOC datasets enter the DA builders unchanged
    (triplet,) = build.build_dataset_da(["voc_s", "voc_t", "voc_a"], None, Catalog, [True, False, False], True)
    assert isinstance(triplet, TripletDataset)
    sample = triplet[0]
    assert sample[1].get_field("is_source").tolist() == [True, True] and sample[3].get_field("is_source").tolist() == [False, False]
    spec = build.dataset_from_spec(("voc:" + root, "trainval"), None, is_train=False, is_source=False)
    assert isinstance(spec, PascalVOCDataset) and spec.keep_difficult is True and spec.is_source is False


def test_evaluate_dispatch_and_aliases(tmp_path, monkeypatch):
    import da_detect_amd.data.evaluation as evaluation
    from da_detect_amd import compat
    from da_detect_amd.data.datasets import ConcatDataset, PascalVOCDataset
    from da_detect_amd.data.evaluation.voc import voc_eval

    root = write_voc_tree(tmp_path, TWO_IMAGES)
    one, two = PascalVOCDataset(root, "test", use_difficult=True), PascalVOCDataset(root, "test", use_difficult=True)
    calls = []
    monkeypatch.setattr(evaluation, "voc_evaluation", lambda **kw: calls.append(kw) or "scored")
    assert evaluation.evaluate(one, ["p"], "out", box_only=False, use_07_metric=False, iou_thresh=[.5, .7]) == "scored"
    assert calls[-1] == dict(dataset=one, predictions=["p"], output_folder="out", box_only=False, use_07_metric=False,
                             iou_thresh=[.5, .7])
    both = ConcatDataset([one, two])
    assert evaluation.evaluate(both, [], None) == "scored" and calls[-1]["dataset"] is both
    view = voc_eval._ConcatView(both)
    assert view.get_groundtruth(3).get_field("labels").tolist() == [2] and view.map_class_id_to_class_name(2) == "bicycle"

    compat.install()
    import maskrcnn_benchmark.data.datasets.evaluation.voc as theirs
    from maskrcnn_benchmark.data.datasets.evaluation.voc import voc_evaluation
    from maskrcnn_benchmark.data.datasets.evaluation.voc.voc_eval import (calc_detection_voc_ap, calc_detection_voc_prec_rec,
                                                                            do_voc_evaluation, eval_detection_voc)
    import da_detect_amd.data.evaluation.voc as ours

    assert theirs is ours and voc_evaluation is ours.voc_evaluation
    assert (calc_detection_voc_ap, calc_detection_voc_prec_rec, do_voc_evaluation, eval_detection_voc) == (
        voc_eval.calc_detection_voc_ap, voc_eval.calc_detection_voc_prec_rec, voc_eval.do_voc_evaluation,
        voc_eval.eval_detection_voc)
