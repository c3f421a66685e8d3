"""COCO box AP on the device: the matching launch (csrc/coco_match.hip) flag for flag, and the numbers end to end, against the
plain loop evaluator and the closed forms of tests/test_coco_eval.py (yardsticks and tolerances are stated there).

Shapes are the smallest at which the kernel can go wrong: pairs with 0, 1, 65, 150 and 300 ground truths (one wave's edge; a
matrix above 64 KiB of LDS, which needs the raised limit; one that no longer fits LDS and lives in the workspace), 110 and
130 detections (the cut to 100, more than one wave filling the matrix), detections without ground truth and the reverse, a
category without ground truth, crowd boxes, equal scores within and across images, IoU exactly at 0.5 / 0.75 / 0.95 and
zero-width boxes."""
import json
import os

import numpy as np
import pytest
import torch

from test_coco_eval import (METRICS, TOL, ListDataset, _coco_files, _images, assert_numbers, closed_form_cases,
                            flags_in_packed_order, loop_box_ap, numbers_from_flags, random_set)

pytestmark = pytest.mark.gpu


def _predictions(dataset, records):
    """the records as the BoxLists they would have come from: xyxy with the "+1" width convention, at the image's own size"""
    from da_detect_amd.structures.bounding_box import BoxList

    to_contiguous = dataset.json_category_id_to_contiguous_id
    out = []
    for index in range(len(dataset.ids)):
        info = dataset.get_img_info(index)
        mine = [r for r in records if r["image_id"] == dataset.id_to_img_map[index]]
        boxes = torch.tensor([[r["bbox"][0], r["bbox"][1], r["bbox"][0] + r["bbox"][2] - 1, r["bbox"][1] + r["bbox"][3] - 1]
                              for r in mine], dtype=torch.float32).reshape(-1, 4)
        box = BoxList(boxes, (info["width"], info["height"]), mode="xyxy")
        box.add_field("scores", torch.tensor([r["score"] for r in mine], dtype=torch.float32))
        box.add_field("labels", torch.tensor([to_contiguous[r["category_id"]] for r in mine], dtype=torch.int64))
        out.append(box)
    return out


@pytest.fixture(scope="module")
def random_case():
    dataset, records = random_set()
    return dataset, records, loop_box_ap(records, dataset)


@pytest.mark.parametrize("name", sorted(closed_form_cases()))
def test_closed_forms_end_to_end(name, tmp_path):
    from da_detect_amd.data.evaluation import evaluate
    from da_detect_amd.data.evaluation.coco.coco_eval import COCOResults

    images, anns, cats, records, want, want_cat, _ = closed_form_cases()[name]
    dataset = _coco_files(tmp_path, images, anns, cats)
    out = str(tmp_path / "out")
    os.makedirs(out)
    results, coco_results = evaluate(dataset, _predictions(dataset, records), out, box_only=False, iou_types=("bbox",),
                                     expected_results=[("bbox", "AP", (want["AP"], .01))], expected_results_sigma_tol=4)
    assert isinstance(results, COCOResults) and list(coco_results) == ["bbox"]
    got = results.results["bbox"]
    loop = loop_box_ap(coco_results["bbox"], dataset)
    for i, m in enumerate(METRICS):
        print(name, m, "device %.12f loop %.12f closed form %.12f" % (got[m], loop["stats"][i], want[m]))
        assert abs(got[m] - want[m]) <= TOL and abs(got[m] - loop["stats"][i]) <= TOL, (name, m, got[m])
    assert sorted(k for k in got if not isinstance(k, str)) == sorted(cats)
    for json_id in cats:
        for i, m in enumerate(METRICS):
            assert abs(got[json_id][m] - loop["per_category"][json_id][i]) <= TOL
            if want_cat:
                assert abs(got[json_id][m] - want_cat[json_id][m]) <= TOL
    # the files: the records as the reference writes them, and the result object
    on_disk = json.load(open(os.path.join(out, "bbox.json")))
    assert on_disk == coco_results["bbox"] and len(on_disk) == len(records)
    for r, w in zip(on_disk, records):          # float32 boxes through the "+1" round trip: these values are exact
        assert (r["image_id"], r["category_id"], r["bbox"]) == (w["image_id"], w["category_id"], w["bbox"])
    saved = torch.load(os.path.join(out, "coco_results.pth"), weights_only=False)
    assert saved.results == results.results


def test_random_set_flags_and_numbers(random_case):
    from da_detect_amd.data.evaluation.coco import box_ap

    dataset, records, loop = random_case
    packed = box_ap.pack(records, dataset)
    matched, ignored, npig = box_ap.match(packed)
    want_m, want_i, want_n = flags_in_packed_order(packed, loop)
    assert matched.is_cuda and matched.dtype == torch.uint8 and tuple(matched.shape) == (10, 4, len(packed.det_score))
    assert torch.equal(npig.cpu(), want_n)
    assert torch.equal(matched.cpu(), want_m), "matched flags differ at %s" % (matched.cpu() != want_m).nonzero()[:5].tolist()
    assert torch.equal(ignored.cpu(), want_i), "ignored flags differ at %s" % (ignored.cpu() != want_i).nonzero()[:5].tolist()
    assert 0 < int(want_m.sum()) < want_m.numel() and 0 < int(want_i.sum()) < want_i.numel()

    # numbers: device accumulation against the loop, and against the same code on CPU tensors
    precision, stats, per_category = numbers_from_flags(packed, matched, ignored, npig)
    assert np.abs(precision - loop["precision"]).max() <= TOL
    assert_numbers(stats, per_category, packed.categories, loop)
    precision_cpu, stats_cpu, per_category_cpu = numbers_from_flags(packed, matched.cpu(), ignored.cpu(), npig.cpu())
    assert np.abs(precision - precision_cpu).max() <= TOL
    assert np.abs(np.array(stats) - np.array(stats_cpu)).max() <= TOL
    assert np.abs(np.array(per_category) - np.array(per_category_cpu)).max() <= TOL
    together, each = box_ap.box_ap(records, dataset)
    assert list(together) == list(METRICS) and list(each) == [3, 5, 9]
    for i, m in enumerate(METRICS):
        print(m, "device %.12f loop %.12f" % (together[m], loop["stats"][i]))
        assert abs(together[m] - loop["stats"][i]) <= TOL
    assert each[9] == dict.fromkeys(METRICS, -1.0)


def test_empty_predictions(tmp_path):
    """No detections at all.  Where there is no ground truth either nothing is launched and all six numbers are -1.  Where
    there is ground truth the launch runs over pairs without detections; by the definition (a cell with
    non-ignored ground truth whose recall never reaches a threshold has precision 0 there) the ranges that have ground truth
    score 0 and the others stay -1 — the loop evaluator says the same."""
    from da_detect_amd.data.evaluation import evaluate

    kwargs = dict(box_only=False, iou_types=("bbox",), expected_results=(), expected_results_sigma_tol=4)
    bare = _coco_files(tmp_path, _images(2), [], [1, 2])
    results, coco_results = evaluate(bare, _predictions(bare, []), None, **kwargs)
    assert coco_results == {"bbox": []}
    assert [results.results["bbox"][m] for m in METRICS] == [-1.0] * 6
    assert results.results["bbox"][1] == dict.fromkeys(METRICS, -1.0)

    images, anns, cats, _, _, _, _ = closed_form_cases()["B"]
    (tmp_path / "b").mkdir()
    dataset = _coco_files(tmp_path / "b", images, anns, cats)
    results, coco_results = evaluate(dataset, _predictions(dataset, []), None, **kwargs)
    loop = loop_box_ap([], dataset)
    assert coco_results == {"bbox": []} and loop["stats"] == [0.0, 0.0, 0.0, -1.0, 0.0, -1.0]
    assert [results.results["bbox"][m] for m in METRICS] == loop["stats"]


def test_malformed_offsets_are_refused_before_the_launch():
    from da_detect_amd import _C, _lib

    dev = torch.device("cuda")
    det = torch.tensor([[0., 0., 10., 10.], [0., 0., 10., 5.], [50., 50., 5., 5.]], dtype=torch.float64, device=dev)
    gt = torch.tensor([[0., 0., 10., 10.], [50., 50., 5., 5.]], dtype=torch.float64, device=dev)
    area = torch.tensor([100., 25.], dtype=torch.float64, device=dev)
    crowd = torch.zeros(2, dtype=torch.int32, device=dev)
    thr, rng = np.linspace(.5, .95, 10), [[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]
    for det_off, gt_off in (([0, 2, 1], [0, 1, 2]), ([0, 2, 10 ** 6], [0, 1, 2]), ([0, 2, 3], [0, 5, 2]), ([1, 2, 3], [0, 1, 2]),
                            ([0, 2, 3], [0, 1, 1]), ([0, -1, 3], [0, 1, 2]), ([0, 2, 3], [0, 1])):
        with pytest.raises(_lib.DadetError) as err:
            _C.coco_match(det, gt, area, crowd, det_off, gt_off, thr, rng)
        assert "status -1" in str(err.value) or "pairs + 1" in str(err.value)
    # nothing faulted: the well-formed table still runs, and gives the obvious answer
    matched, ignored, npig = _C.coco_match(det, gt, area, crowd, [0, 2, 3], [0, 1, 2], thr, rng)
    torch.cuda.synchronize()
    assert npig.tolist() == [[1, 1, 0, 0], [1, 1, 0, 0]]
    assert matched[:, 0, :].tolist() == [[1, 0, 1]] * 10             # the exact box takes the ground truth, IoU 0.5 comes second
    assert ignored[:, 0, :].tolist() == [[0, 0, 0]] * 10 and ignored[0, 2, :].tolist() == [1, 1, 1]


def test_score_tool_on_saved_predictions(tmp_path):
    """tools/score_net_da.py on a predictions.pth as tools/test_net_da.py leaves it: case B's table and files"""
    import subprocess
    import sys

    images, anns, cats, records, want, _, _ = closed_form_cases()["B"]
    dataset = _coco_files(tmp_path, images, anns, cats)
    saved = os.path.join(str(tmp_path), "predictions.pth")
    torch.save(_predictions(dataset, records), saved)
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "score_net_da.py")
    res = subprocess.run([sys.executable, tool, "--dataset", os.path.join(str(tmp_path), "ann.json") + "," + str(tmp_path),
                          "--predictions", saved], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "3 detections on 1 images" in res.stderr and "%8.3f" % want["AP"] in res.stderr
    got = torch.load(os.path.join(str(tmp_path), "coco_results.pth"), weights_only=False).results["bbox"]
    for m in METRICS:
        assert abs(got[m] - want[m]) <= TOL and abs(got[1][m] - want[m]) <= TOL
    assert len(json.load(open(os.path.join(str(tmp_path), "bbox.json")))) == 3


def test_concat_dataset_end_to_end(tmp_path):
    """case D with its two images in two COCODatasets, concatenated: the same numbers as in one dataset"""
    from da_detect_amd.data.datasets import ConcatDataset
    from da_detect_amd.data.evaluation import evaluate

    images, anns, cats, records, want, _, _ = closed_form_cases()["D"]
    parts = []
    for k, im in enumerate(images):
        (tmp_path / str(k)).mkdir()
        parts.append(_coco_files(tmp_path / str(k), [im], [a for a in anns if a["image_id"] == im["id"]], cats))
    predictions = [p for part in parts for p in _predictions(part, records)]
    results, _ = evaluate(ConcatDataset(parts), predictions, None, box_only=False, iou_types=("bbox",), expected_results=(),
                          expected_results_sigma_tol=4)
    for m in METRICS:
        assert abs(results.results["bbox"][m] - want[m]) <= TOL, m


@pytest.mark.parametrize("rpn_only", [False, True])
def test_score_tool_evaluates_and_scores_in_one_command(rpn_only, tmp_path):
    """tools/score_net_da.py --config-file: the evaluation pass of tools/test_net_da.py (seeded random weights, tiny images) and
    the scoring in one command — the box AP table, or with MODEL.RPN_ONLY the proposal recalls, which the evaluation pass
    itself now reaches instead of failing on proposals without scores"""
    import subprocess
    import sys

    from test_data_pipeline import _write_coco

    ann, folder = _write_coco(str(tmp_path), "target", 3, np.random.default_rng(1), sizes=[(96, 192), (80, 160), (96, 128)])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "out")
    os.makedirs(out)
    run = [sys.executable, os.path.join(root, "tools", "score_net_da.py"), "--dataset", ann + "," + folder, "--config-file",
           os.path.join(root, "configs/da_faster_rcnn/e2e_da_faster_rcnn_R_50_C4_cityscapes_to_foggy_cityscapes.yaml"),
           "--output-dir", out, "DATALOADER.NUM_WORKERS", "0", "INPUT.MIN_SIZE_TEST", "96", "INPUT.MAX_SIZE_TEST", "192",
           "MODEL.WEIGHT", "", "MODEL.ROI_BOX_HEAD.NUM_CLASSES", "3", "MODEL.ROI_HEADS.SCORE_THRESH", "0.0"]
    res = subprocess.run(run + (["MODEL.RPN_ONLY", "True"] if rpn_only else []), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    where = os.path.join(out, "inference", "target")
    assert os.path.exists(os.path.join(where, "predictions.pth"))
    if rpn_only:
        got = torch.load(os.path.join(where, "box_proposals.pth"), weights_only=False).results["box_proposal"]
        assert sorted(got) == sorted(["AR@100", "ARs@100", "ARm@100", "ARl@100", "AR@1000", "ARs@1000", "ARm@1000", "ARl@1000"])
        assert 0.0 <= got["AR@1000"] <= 1.0 and res.stderr.count("Evaluating bbox proposals") == 2       # the pass, then the tool
    else:
        got = torch.load(os.path.join(where, "coco_results.pth"), weights_only=False).results["bbox"]
        records = json.load(open(os.path.join(where, "bbox.json")))
        assert len(records) > 0 and sorted(k for k in got if not isinstance(k, str)) == [24, 26]
        assert all(-1.0 <= got[m] <= 1.0 for m in METRICS) and got["AP"] >= 0.0 and got["APl"] == -1.0   # areas are 300: small
        assert "COCO box AP" in res.stderr and "%d detections on 3 images" % len(records) in res.stderr
