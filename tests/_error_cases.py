"""Yardsticks and cases of the error breakdown; a helper, not collected by pytest.

  * `loop_errors`: the rule, plainly — one Python loop per image, IoU from numpy float32 scalars in the stated operation order
    (`iou32`), claims made by walking the detections in rank order.  Images with many ground truths use `iou32_row`, the same
    expressions on float32 arrays (one detection against all ground truths); the host tests pin the two together bit for bit.
  * `loop_summary`: the fixes and their APs as plain float64 loops over `loop_ap` of tests/test_voc_eval.py; a dropped
    detection is really removed from its class's list (the package flags it -1 instead).
  * the case builders.

All arrays are in the package's packed order: images ascending, inside an image descending score, ties in record order."""
import numpy as np

from test_voc_eval import loop_ap, pred, truth

TP, IGNORED, CLS, LOC, BOTH, DUPE, BKG = range(7)
DETECTED, DIFFICULT, COVERED, MISSED = range(4)
FIXES = ("Cls", "Loc", "Both", "Dupe", "Bkg", "Miss", "FP", "FN")
F = np.float32


def iou32(d, g):
    """float32 "+1" IoU of csrc/voc_match.hip: x2, y2 raised by 1, the "+1" areas, inter / ((area_d + area_g) - inter)"""
    one, zero = F(1), F(0)
    dx1, dy1, dx2, dy2 = F(d[0]), F(d[1]), F(d[2]) + one, F(d[3]) + one
    gx1, gy1, gx2, gy2 = F(g[0]), F(g[1]), F(g[2]) + one, F(g[3]) + one
    da = (dx2 - dx1 + one) * (dy2 - dy1 + one)
    ga = (gx2 - gx1 + one) * (gy2 - gy1 + one)
    w = max(min(dx2, gx2) - max(dx1, gx1) + one, zero)
    h = max(min(dy2, gy2) - max(dy1, gy1) + one, zero)
    inter = w * h
    out = inter / ((da + ga) - inter)
    assert type(out) is np.float32
    return out


def iou32_row(d, gts):
    """`iou32` of one detection against float32 [G, 4] ground truths: the same operations, elementwise"""
    one, zero = F(1), F(0)
    d, gts = np.asarray(d, dtype=F), np.asarray(gts, dtype=F).reshape(-1, 4)
    dx1, dy1, dx2, dy2 = d[0], d[1], d[2] + one, d[3] + one
    gx1, gy1, gx2, gy2 = gts[:, 0], gts[:, 1], gts[:, 2] + one, gts[:, 3] + one
    da = (dx2 - dx1 + one) * (dy2 - dy1 + one)
    ga = (gx2 - gx1 + one) * (gy2 - gy1 + one)
    w = np.maximum(np.minimum(dx2, gx2) - np.maximum(dx1, gx1) + one, zero)
    h = np.maximum(np.minimum(dy2, gy2) - np.maximum(dy1, gy1) + one, zero)
    inter = w * h
    out = inter / ((da + ga) - inter)
    assert out.dtype == np.float32
    return out


def reaches(v, t):
    """ "v >= t" as the kernel reads it"""
    return not (float(v) < t)


def fp_kind(s, o, tf, tb):
    if reaches(s, tb) and not reaches(s, tf):
        return LOC
    if reaches(o, tf):
        return CLS
    if reaches(s, tf):
        return DUPE
    if not reaches(s, tb) and not reaches(o, tb):
        return BKG
    return BOTH


def loop_errors(preds, gts, pos_thresh=0.5, bg_thresh=0.1, scalar_limit=40000):
    """-> dict of numpy arrays in packed order: det_kind, det_gt, iou_same, iou_other, det_fix, gt_state, gt_det, and the
    inputs as packed (det_label, det_score, gt_label, gt_difficult, det_off, gt_off, det_order)"""
    tf, tb = float(pos_thresh), float(bg_thresh)
    out = {k: [] for k in ("det_kind", "det_gt", "iou_same", "iou_other", "det_fix", "gt_state", "gt_det", "det_label",
                           "det_score", "gt_label", "gt_difficult", "det_order")}
    det_off, gt_off = [0], [0]
    for p, g in zip(preds, gts):
        d0, g0 = det_off[-1], gt_off[-1]
        boxes, labels = p.bbox.numpy().astype(F), p.get_field("labels").numpy().astype(np.int64)
        scores = p.get_field("scores").numpy().astype(F).astype(np.float64)
        gbox, glabel = g.bbox.numpy().astype(F), g.get_field("labels").numpy().astype(np.int64)
        hard = g.get_field("difficult").numpy().astype(bool)
        order = np.argsort(-scores, kind="stable")
        D, G = len(order), len(glabel)
        maxima = []
        for r in order:
            if D * G > scalar_limit:
                row = iou32_row(boxes[r], gbox)
            else:
                row = [iou32(boxes[r], gbox[j]) for j in range(G)]
            best = {"cand": (F(0), -1), "s": (F(0), -1), "o": (F(0), -1)}

            def offer(name, v, j):
                if best[name][1] < 0 or v > best[name][0]:
                    best[name] = (v, j)

            for j in range(G):
                if glabel[j] == labels[r]:
                    offer("cand", row[j], j)
                    if not hard[j]:
                        offer("s", row[j], j)
                elif not hard[j]:
                    offer("o", row[j], j)
            maxima.append(best)

        kind, target = [None] * D, [-1] * D
        owner = {}                                              # ground truth -> rank of its TP
        for d, best in enumerate(maxima):                       # rank order: the first to come takes the ground truth
            v, j = best["cand"]
            if j >= 0 and reaches(v, tf):
                target[d] = j
                if hard[j]:
                    kind[d] = IGNORED
                elif j not in owner:
                    kind[d] = TP
                    owner[j] = d
        for d, best in enumerate(maxima):
            if kind[d] is not None:
                continue
            kind[d] = fp_kind(best["s"][0], best["o"][0], tf, tb)
            target[d] = {LOC: best["s"][1], CLS: best["o"][1], BOTH: best["o"][1], DUPE: best["cand"][1], BKG: -1}[kind[d]]
        fix, claimed = [0] * D, {LOC: set(), CLS: set()}
        for d in range(D):
            if kind[d] in (LOC, CLS) and target[d] not in owner and target[d] not in claimed[kind[d]]:
                fix[d] = 1
                claimed[kind[d]].add(target[d])
        pointed = set(target[d] for d in range(D) if kind[d] in (LOC, CLS))
        for j in range(G):
            state = DIFFICULT if hard[j] else DETECTED if j in owner else COVERED if j in pointed else MISSED
            out["gt_state"].append(state)
            out["gt_det"].append(d0 + owner[j] if state == DETECTED else -1)
        out["det_kind"].extend(kind)
        out["det_gt"].extend(g0 + j if j >= 0 else -1 for j in target)
        out["iou_same"].extend(best["s"][0] for best in maxima)
        out["iou_other"].extend(best["o"][0] for best in maxima)
        out["det_fix"].extend(fix)
        out["det_label"].extend(labels[order].tolist())
        out["det_score"].extend(scores[order].tolist())
        out["det_order"].extend((d0 + order).tolist())
        out["gt_label"].extend(glabel.tolist())
        out["gt_difficult"].extend(hard.astype(np.uint8).tolist())
        det_off.append(d0 + D)
        gt_off.append(g0 + G)
    dtypes = dict(det_kind=np.uint8, det_gt=np.int32, iou_same=F, iou_other=F, det_fix=np.uint8, gt_state=np.uint8,
                  gt_det=np.int32, det_label=np.int64, det_score=np.float64, gt_label=np.int64, gt_difficult=np.uint8,
                  det_order=np.int64)
    out = {k: np.array(v, dtype=dtypes[k]) for k, v in out.items()}
    out["det_off"], out["gt_off"] = np.array(det_off, dtype=np.int32), np.array(gt_off, dtype=np.int32)
    return out


def _class_ap(flags, labels, scores, n_pos, present, use_07_metric):
    """flags in {-1 ignored, 0, 1}, None = dropped -> AP per class by `loop_ap`, nan for absent classes / no positives"""
    K = len(n_pos)
    prec, rec = [None] * K, [None] * K
    for k in range(K):
        if not present[k]:
            continue
        mine = [i for i in range(len(flags)) if labels[i] == k and flags[i] is not None]
        mine.sort(key=lambda i: -scores[i])                       # stable: ties keep the packed order
        m = np.array([flags[i] for i in mine], dtype=np.int64)
        tp, fp = np.cumsum(m == 1), np.cumsum(m == 0)
        with np.errstate(invalid="ignore", divide="ignore"):
            prec[k] = tp / (fp + tp)
            if n_pos[k] > 0:
                rec[k] = tp / float(n_pos[k])
    return loop_ap(prec, rec, use_07_metric)


def _mean(ap):
    kept = [v for v in ap if v == v]
    return sum(kept) / len(kept) if kept else float("nan")


def loop_summary(loop, K, use_07_metric=False):
    """the numbers `errors.summarise` gives, from plain loops over `loop_errors`' arrays (or hand-made ones of that form)"""
    kind, fix, target = loop["det_kind"].tolist(), loop["det_fix"].tolist(), loop["det_gt"].tolist()
    label, score = loop["det_label"].tolist(), loop["det_score"].tolist()
    glabel, state = loop["gt_label"].tolist(), loop["gt_state"].tolist()
    n = len(kind)
    present = [k in set(label) | set(glabel) for k in range(K)]
    counts = np.zeros((K, 7), dtype=np.int64)
    confusion = np.zeros((K, K + 1), dtype=np.int64)
    for i in range(n):
        counts[label[i], kind[i]] += 1
        if kind[i] != IGNORED:
            confusion[label[i], glabel[target[i]] if target[i] >= 0 else K] += 1
    per_state = {s: np.zeros(K, dtype=np.int64) for s in range(4)}
    for j in range(len(glabel)):
        per_state[state[j]][glabel[j]] += 1
    n_pos = per_state[DETECTED] + per_state[COVERED] + per_state[MISSED]
    missed = per_state[MISSED]

    base = [1 if k == TP else -1 if k == IGNORED else 0 for k in kind]
    ap = _class_ap(base, label, score, n_pos, present, use_07_metric)

    def claim_fixed(which):
        return [(1 if fix[i] else None) if kind[i] == which else base[i] for i in range(n)]

    def without(which):
        return [None if kind[i] == which else base[i] for i in range(n)]

    moved = [glabel[target[i]] if kind[i] == CLS and fix[i] else label[i] for i in range(n)]
    scenarios = {"Cls": (claim_fixed(CLS), moved, n_pos), "Loc": (claim_fixed(LOC), label, n_pos),
                 "Both": (without(BOTH), label, n_pos), "Dupe": (without(DUPE), label, n_pos), "Bkg": (without(BKG), label, n_pos),
                 "Miss": (base, label, n_pos - missed), "FP": ([None if b == 0 else b for b in base], label, n_pos),
                 "FN": (base, label, per_state[DETECTED])}
    dap, dap_by_class = {}, {}
    for name, (flags, labels, pos) in scenarios.items():
        fixed = _class_ap(flags, labels, score, pos, present, use_07_metric)
        dap[name] = _mean(fixed) - _mean(ap)
        dap_by_class[name] = fixed - ap

    top = np.full((K, 3), np.nan)
    for k in range(K):
        mine = [i for i in range(n) if label[i] == k and kind[i] != IGNORED]
        mine.sort(key=lambda i: -score[i])
        mine = mine[:int(n_pos[k])]
        if mine:
            right, loc = sum(kind[i] == TP for i in mine), sum(kind[i] == LOC for i in mine)
            top[k] = [right / len(mine), loc / len(mine), (len(mine) - right - loc) / len(mine)]
    return {"counts": counts, "missed": missed, "covered": per_state[COVERED], "n_pos": n_pos, "confusion": confusion, "ap": ap,
            "map": _mean(ap), "dap": dap, "dap_by_class": dap_by_class, "top_ranked": top}


# ------------------------------------------------------------------------------------------------ cases
BOX = [10, 10, 50, 40]
SHIFTED = [34, 10, 74, 40]          # on BOX: 18 * 32 of 2 * 42 * 32 - 18 * 32, IoU 0.27: between the two thresholds
NONE = np.zeros((0, 4))


def edge_images():
    """-> list of (what, pred, truth, expected det_kind in rank order or None, expected det_fix or None)"""
    return [
        ("no detections", pred(NONE, [], []), truth([BOX], [1]), [], []),
        ("no ground truth", pred([BOX, [0, 0, 5, 5]], [1, 2], [.9, .8]), truth(NONE, []), [BKG, BKG], [0, 0]),
        ("one of each", pred([BOX], [1], [.9]), truth([BOX], [1]), [TP], [0]),
        ("two identical ground truths", pred([BOX, BOX, BOX], [1, 1, 1], [.9, .8, .7]), truth([BOX, BOX], [1, 1]),
         [TP, DUPE, DUPE], [0, 0, 0]),
        ("a difficult ground truth claimed twice", pred([BOX, [11, 10, 50, 40]], [1, 1], [.9, .5]), truth([BOX], [1], [1]),
         [IGNORED, IGNORED], [0, 0]),
        ("difficult in front of an easier one", pred([BOX], [1], [.9]), truth([BOX, [10, 10, 50, 30]], [1, 1], [1, 0]),
         [IGNORED], [0]),
        # the second detection repeats the first (Dupe-eligible) and sits on another class's box as well: Cls comes first
        ("Dupe-eligible and Cls-eligible", pred([BOX, BOX], [1, 1], [.9, .8]), truth([BOX, BOX], [1, 2]), [TP, CLS], [0, 1]),
        ("two Loc on one undetected ground truth", pred([SHIFTED, SHIFTED], [1, 1], [.9, .8]), truth([BOX], [1]),
         [LOC, LOC], [1, 0]),
        ("a Loc and a Cls on one ground truth", pred([SHIFTED, BOX], [1, 2], [.9, .8]), truth([BOX], [1]), [LOC, CLS], [1, 1]),
        ("a Loc on a detected ground truth", pred([BOX, SHIFTED], [1, 1], [.9, .8]), truth([BOX], [1]), [TP, LOC], [0, 0]),
        ("Both: wrong class, badly placed", pred([SHIFTED], [2], [.9]), truth([BOX], [1]), [BOTH], [0]),
        ("equal scores keep the record order", pred([BOX, BOX], [1, 1], [.5, .5]), truth([BOX], [1]), [TP, DUPE], [0, 0]),
    ]


def threshold_images():
    """IoU exactly at both thresholds.  With x2, y2 raised by 1 AND the "+1" areas a box (0, 0, a, b) weighs (a + 2)(b + 2):
    (0, 0, 8, 8) weighs 100; (0, 0, 8, 3) inside it 50 -> exactly 0.5; (0, 0, 3, 0) 10 -> exactly float32 0.1; (0, 0, 1, 1)
    9 -> 0.09.  The last three are the issue's own coordinates, which presume one "+1": under the pinned expression (0, 0, 9, 9)
    weighs 121 and they come to 66 / 121, 22 / 121 and 20 / 121; they stay in, compared with the loop.
    -> list of (what, pred, truth, expected kind, expected iou_same or None)"""
    d8, d9 = [0, 0, 8, 8], [0, 0, 9, 9]
    return [
        ("exactly 0.5", pred([d8], [1], [.9]), truth([[0, 0, 8, 3]], [1]), TP, F(0.5)),
        ("exactly float32 0.1", pred([d8], [1], [.9]), truth([[0, 0, 3, 0]], [1]), LOC, F(0.1)),
        ("0.09", pred([d8], [1], [.9]), truth([[0, 0, 1, 1]], [1]), BKG, F(9) / F(100)),
        ("(0,0,9,9) on (0,0,9,4)", pred([d9], [1], [.9]), truth([[0, 0, 9, 4]], [1]), TP, F(66) / F(121)),
        ("(0,0,9,9) on (0,0,9,0)", pred([d9], [1], [.9]), truth([[0, 0, 9, 0]], [1]), LOC, F(22) / F(121)),
        ("(0,0,9,9) on (0,0,8,0)", pred([d9], [1], [.9]), truth([[0, 0, 8, 0]], [1]), LOC, F(20) / F(121)),
    ]


def crowded(rng, n_det, n_gt, n_class=3, size=(640, 480)):
    """ground truths on a jittered grid with labels 1..n_class, about a fifth difficult; detections are jittered copies
    (sigma 2.5) of random ground truths with their labels, a quarter jittered further (sigma 12), a fifth given a random label,
    15 % replaced by large random boxes; distinct scores"""
    cols = int(np.ceil(np.sqrt(n_gt * size[0] / size[1])))
    rows = int(np.ceil(n_gt / cols))
    cw, ch = size[0] / cols, size[1] / rows
    cell = np.arange(n_gt)
    gx = (cell % cols) * cw + rng.uniform(0, .3 * cw, n_gt)
    gy = (cell // cols) * ch + rng.uniform(0, .3 * ch, n_gt)
    gts = np.stack([gx, gy, gx + rng.uniform(.35 * cw, .65 * cw, n_gt), gy + rng.uniform(.35 * ch, .65 * ch, n_gt)], 1)
    glabel = rng.integers(1, n_class + 1, n_gt)
    hard = rng.uniform(size=n_gt) < .2
    pick = rng.integers(0, n_gt, n_det)
    dets = gts[pick] + rng.normal(0, 2.5, (n_det, 4))
    further = rng.uniform(size=n_det) < .25
    dets[further] += rng.normal(0, 12, (int(further.sum()), 4))
    labels = glabel[pick].copy()
    relabel = rng.uniform(size=n_det) < .2
    labels[relabel] = rng.integers(1, n_class + 1, int(relabel.sum()))
    large = rng.uniform(size=n_det) < .15
    m = int(large.sum())
    dets[large] = np.stack([rng.uniform(0, .45 * size[0], m), rng.uniform(0, .45 * size[1], m),
                            rng.uniform(.5 * size[0], size[0] - 1, m), rng.uniform(.5 * size[1], size[1] - 1, m)], 1)
    dets[:, 2:] = np.maximum(dets[:, 2:], dets[:, :2] + 1)
    scores = (rng.permutation(n_det) + 1.0) / (n_det + 1)
    return pred(dets, labels, scores, size), truth(gts, glabel, hard, size)
