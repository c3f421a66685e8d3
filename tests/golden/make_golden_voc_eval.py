"""Golden record for PASCAL VOC AP — runs ONLY in the authoring container (needs /root/reference).

Calls the reference's own `calc_detection_voc_prec_rec` and `calc_detection_voc_ap`
(maskrcnn_benchmark/data/datasets/evaluation/voc/voc_eval.py) on a seeded synthetic set and stores DATA ONLY in
tests/golden/voc_eval_cases.npz:

  * the inputs: per image its size, detections (float32 xyxy boxes, labels, scores) and ground truths (boxes, labels,
    difficult), concatenated with the image index of every row;
  * at IoU 0.5 and 0.75 (both exact in binary, so a float32 IoU compares the same against the float32 and the float64
    threshold): per label `prec` and `rec`, concatenated, with offsets and a "present" mask for the None holes;
  * `n_pos` per label, AP for both metrics (11-point, area) at both thresholds, and their nanmean.

The set: 40 images, labels from {1, 2, 3, 5, 6} (0 and 4 are never used: None holes), about 600 detections that are jittered
copies of ground truths plus random boxes, non-integer float32 coordinates, about 15 % of the ground truths difficult, label
6 with difficult ground truths only on top of that (n_pos == 0: AP nan), images without ground truth of a class, one image without
detections, one without ground truth.  Scores are a random permutation of k / N, all distinct (asserted), so the
reference's unstable tie order cannot matter.

The reference's package __init__ files pull in torchvision; the packages are registered as bare namespaces over the
reference's directories (as make_golden_box_proposals.py does), so only voc_eval.py, structures/bounding_box.py and
structures/boxlist_ops.py are executed.

    python tests/golden/make_golden_voc_eval.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import ref_shims  # noqa: E402

THRESHOLDS = (0.5, 0.75)
LABELS = (1, 2, 3, 5, 6)
ONLY_DIFFICULT = 6


def _bare_packages(ref_c):
    base = os.path.join(ref_shims.REF_ROOT, "maskrcnn_benchmark")
    for name in [n for n in sys.modules if n == "maskrcnn_benchmark" or n.startswith("maskrcnn_benchmark.")]:
        del sys.modules[name]
    for sub in ("", ".structures", ".data", ".data.datasets", ".data.datasets.evaluation", ".data.datasets.evaluation.voc"):
        m = types.ModuleType("maskrcnn_benchmark" + sub)
        m.__path__ = [os.path.join(base, *[p for p in sub.split(".") if p])]
        sys.modules[m.__name__] = m
    layers = types.ModuleType("maskrcnn_benchmark.layers")
    layers.nms = ref_c.nms
    sys.modules.update({"maskrcnn_benchmark.layers": layers, "maskrcnn_benchmark._C": ref_c})


def make_inputs(seed=7, n_img=40):
    rng = np.random.default_rng(seed)
    W, H = 640, 480
    det, gt = [], []          # rows (image, label, x1, y1, x2, y2[, difficult])
    for i in range(n_img):
        mine = []
        if i != 5:                                                # image 5: no ground truth at all
            for _ in range(int(rng.integers(3, 9))):
                label = LABELS[int(rng.integers(len(LABELS)))]
                w, h = rng.uniform(20, 200), rng.uniform(20, 160)
                x, y = rng.uniform(0, W - w - 1), rng.uniform(0, H - h - 1)
                difficult = label == ONLY_DIFFICULT or rng.uniform() < .15
                mine.append((i, label, x, y, x + w, y + h, difficult))
        gt.extend(mine)
        n = 0 if i == 9 else int(rng.integers(12, 19))          # image 9: no detections
        for k in range(n):
            if mine and k % 4 != 3:
                _, label, x1, y1, x2, y2, _ = mine[int(rng.integers(len(mine)))]
                s = (.03, .08, .15)[k % 3]
                w, h = x2 - x1, y2 - y1
                x1, x2 = x1 + w * rng.normal(0, s), x2 + w * rng.normal(0, s)
                y1, y2 = y1 + h * rng.normal(0, s), y2 + h * rng.normal(0, s)
                if rng.uniform() < .1:
                    label = LABELS[int(rng.integers(len(LABELS)))]
            else:
                label = LABELS[int(rng.integers(len(LABELS)))]
                x1, y1 = rng.uniform(0, W - 60), rng.uniform(0, H - 60)
                x2, y2 = x1 + rng.uniform(10, 200), y1 + rng.uniform(10, 160)
            x1, y1, x2, y2 = max(x1, 0.), max(y1, 0.), min(max(x2, x1 + 2), W - 1.), min(max(y2, y1 + 2), H - 1.)
            det.append((i, label, x1, y1, x2, y2))
    det, gt = np.array(det, dtype=np.float64), np.array(gt, dtype=np.float64)
    n = len(det)
    score = (rng.permutation(n).astype(np.float64) + 1) / (n + 1)
    out = dict(image_size=np.array([[W, H]] * n_img, dtype=np.int64),
               det_image=det[:, 0].astype(np.int64), det_label=det[:, 1].astype(np.int64),
               det_box=det[:, 2:6].astype(np.float32), det_score=score.astype(np.float32),
               gt_image=gt[:, 0].astype(np.int64), gt_label=gt[:, 1].astype(np.int64), gt_box=gt[:, 2:6].astype(np.float32),
               gt_difficult=gt[:, 6].astype(np.uint8))
    assert len(np.unique(out["det_score"])) == n, "float32 scores collide: the tie order would matter"
    return out


def boxlists(inp, BoxList):
    preds, gts = [], []
    for i, (w, h) in enumerate(inp["image_size"].tolist()):
        d, g = inp["det_image"] == i, inp["gt_image"] == i
        p = BoxList(torch.from_numpy(inp["det_box"][d]).reshape(-1, 4), (w, h), mode="xyxy")
        p.add_field("labels", torch.from_numpy(inp["det_label"][d]))
        p.add_field("scores", torch.from_numpy(inp["det_score"][d]))
        t = BoxList(torch.from_numpy(inp["gt_box"][g]).reshape(-1, 4), (w, h), mode="xyxy")
        t.add_field("labels", torch.from_numpy(inp["gt_label"][g]))
        t.add_field("difficult", torch.from_numpy(inp["gt_difficult"][g]))
        preds.append(p)
        gts.append(t)
    return preds, gts


def _flat(curves):
    present = np.array([c is not None for c in curves], dtype=bool)
    parts = [np.asarray(c, dtype=np.float64) for c in curves if c is not None]
    off = np.cumsum([0] + [len(c) if c is not None else 0 for c in curves]).astype(np.int64)
    return (np.concatenate(parts) if parts else np.zeros(0)), off, present


def main():
    _bare_packages(ref_shims.install())
    from maskrcnn_benchmark.data.datasets.evaluation.voc import voc_eval as ref
    from maskrcnn_benchmark.structures.bounding_box import BoxList as RefBoxList

    assert ref.__file__.startswith("/root/reference")
    inp = make_inputs()
    preds, gts = boxlists(inp, RefBoxList)
    K = max(LABELS) + 1
    out = dict(inp)
    out["thresholds"] = np.array(THRESHOLDS, dtype=np.float64)
    out["n_pos"] = np.array([int(((inp["gt_label"] == k) & (inp["gt_difficult"] == 0)).sum()) for k in range(K)], dtype=np.int64)
    ap, mean = np.zeros((len(THRESHOLDS), 2, K)), np.zeros((len(THRESHOLDS), 2))
    with np.errstate(invalid="ignore", divide="ignore"):
        for t, thr in enumerate(THRESHOLDS):
            prec, rec = ref.calc_detection_voc_prec_rec(pred_boxlists=preds, gt_boxlists=gts, iou_thresh=thr)
            assert len(prec) == K and prec[0] is None and prec[4] is None and rec[ONLY_DIFFICULT] is None
            assert prec[ONLY_DIFFICULT] is not None
            for name, curves in (("prec", prec), ("rec", rec)):
                flat, off, present = _flat(curves)
                out["%s_%d" % (name, t)], out["%s_off_%d" % (name, t)], out["%s_present_%d" % (name, t)] = flat, off, present
            for m, use_07 in enumerate((True, False)):
                ap[t, m] = ref.calc_detection_voc_ap(prec, rec, use_07_metric=use_07)
                mean[t, m] = np.nanmean(ap[t, m])
                again = ref.eval_detection_voc(preds, gts, iou_thresh=thr, use_07_metric=use_07)
                assert np.array_equal(again["ap"], ap[t, m], equal_nan=True) and again["map"] == mean[t, m]
            print("IoU %.2f: mAP 11-point %.6f, area %.6f; AP %s" % (thr, mean[t, 0], mean[t, 1], np.round(ap[t, 0], 4)))
    assert np.isnan(ap[:, :, [0, 4, ONLY_DIFFICULT]]).all() and not np.isnan(ap[:, :, [1, 2, 3, 5]]).any()
    assert (ap[0] != ap[1])[:, [1, 2, 3, 5]].any(), "the two thresholds give the same AP: jitter the detections more"
    out["ap"], out["map"] = ap, mean           # [threshold, (11-point, area), label], [threshold, metric]
    path = os.path.join(HERE, "voc_eval_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes): %d detections, %d ground truths, n_pos %s" % (path, os.path.getsize(path), len(inp["det_score"]),
                                                                              len(inp["gt_label"]), out["n_pos"].tolist()))


if __name__ == "__main__":
    main()
