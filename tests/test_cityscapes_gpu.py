"""csrc/instance_boxes.hip against the host statement of the rules (data/cityscapes.py instance_table_host, itself pinned
against an independent evaluator in test_cityscapes_host.py).  Every comparison is integer equality.  The kernel's tile is
TILE_H x TILE_W pixels per workgroup, walked in row segments of SEGMENT pixels (one wave); the cases below sit on those
edges, on packed maps of odd width (rows at odd 2-byte offsets) and on the batch size of a split."""
import json
import os

import numpy as np
import pytest

from da_detect_amd.data import cityscapes as cs
from test_cityscapes_host import assert_balanced, blob_map, blob_maps, load_converter, make_tree

pytestmark = pytest.mark.gpu

TW, TH, SEG = cs.TILE_W, cs.TILE_H, cs.SEGMENT


def host(maps):
    return [cs.instance_table_host(m).tolist() for m in maps]


def device(maps):
    return [t.tolist() for t in cs.instance_table_device(maps, "cuda")]


def check(maps):
    expected = host(maps)
    got = device(maps)
    assert len(got) == len(expected)
    for i, (g, e) in enumerate(zip(got, expected)):
        assert g == e, "map %d (%s)" % (i, "x".join(str(s) for s in np.asarray(maps[i]).shape))
    return expected


def test_mixed_sizes_in_one_batch():
    """1x1 .. 64x300 packed back to back: after the 1x7 map every row of the 5x65 and 33x257 maps starts at an odd offset"""
    maps = [blob_map(20 + i, H, W, instances=6) for i, (H, W) in enumerate([(1, 1), (1, 7), (7, 1), (5, 65), (33, 257), (64, 300)])]
    maps[0][0, 0] = 26001
    maps[1][0, 2:5] = 24001
    maps[2][1:4, 0] = 25001
    expected = check(maps)
    assert expected[0] == [[26001, 0, 0, 0, 0, 1, 1]] and [24001, 2, 0, 4, 0, 3, 0] in expected[1]
    assert sum(len(t) for t in expected) > 10


def test_empty_map_and_one_instance_map():
    empty = np.full((40, 70), 7, np.uint16)
    full = np.full((TH + 3, TW + 5), 26001, np.uint16)
    expected = check([empty, full, empty])
    assert expected == [[], [[26001, 0, 0, TW + 4, TH + 2, (TH + 3) * (TW + 5), 0]], []]


def test_run_across_every_segment_tile_and_workgroup_boundary():
    """one row run over 2 tiles and a bit (9 segments), and a column run over 3 row bands"""
    ids = np.full((3 * TH + 2, 2 * TW + SEG // 2), 8, np.uint16)
    ids[TH - 1, 1:-1] = 27001
    ids[1:-1, TW] = 27001
    ids[TH:TH + 2, TW - 1:TW + 1] = 28002                       # a 2 x 2 block on the corner of four tiles
    expected = check([ids])
    assert [row[:5] for row in expected[0]] == [[27001, 1, 1, 2 * TW + SEG // 2 - 2, 3 * TH], [28002, TW - 1, TH, TW, TH + 1]]
    assert [row[6] for row in expected[0]] == [0, 0]


def test_one_id_in_two_far_corners():
    ids = np.zeros((2 * TH + 5, 3 * TW + 7), np.uint16)
    ids[0:2, 0:2] = 31005
    ids[-2:, -2:] = 31005
    assert check([ids]) == [[[31005, 0, 0, 3 * TW + 6, 2 * TH + 4, 8, 0]]]


def test_two_pixel_pairs_on_tile_edges_and_image_border():
    ids = np.full((2 * TH + 4, 2 * TW + 4), 11, np.uint16)
    ids[TH - 1, TW - 1] = ids[TH, TW] = 24001                   # diagonal pair over a tile corner
    ids[TH - 1, 40] = ids[TH, 39] = 24002                       # anti-diagonal pair over a workgroup's row band
    ids[5, TW - 1] = ids[5, TW] = 24003                         # horizontal pair over a tile's column edge
    ids[7, SEG - 1] = ids[7, SEG] = 24004                       # ... and over a segment edge inside a tile
    ids[0, 100] = ids[0, 101] = 24005                           # pairs on the image border
    ids[-1, -1] = ids[-2, -1] = 24006
    ids[20, 0] = ids[21, 0] = 24007
    ids[TH - 1, 2 * TW - 1] = ids[TH, 2 * TW] = ids[TH + 1, 2 * TW + 1] = 25001      # three on a diagonal over a corner: whole
    ids[2 * TH - 2:2 * TH + 1, 70] = 25002                      # three down a column over a row band: whole
    ids[2, 2:12] = ids[TH + 7, 200] = 25003                     # a body and a far single pixel
    expected = check([ids])
    assert [(row[0], row[5], row[6]) for row in expected[0]] == [
        (24001, 2, 1), (24002, 2, 1), (24003, 2, 1), (24004, 2, 1), (24005, 2, 1), (24006, 2, 1), (24007, 2, 1),
        (25001, 3, 0), (25002, 3, 0), (25003, 11, 1)]


def test_slot_edges():
    ids = np.zeros((9, 50), np.uint16)
    for k, value in enumerate((23999, 24000, 24999, 33000, 33999, 34000, 999, 65535)):
        ids[2:6, 6 * k:6 * k + 4] = value
    expected = check([ids])
    assert [row[0] for row in expected[0]] == [24000, 24999, 33000, 33999]


def test_more_ids_than_the_workgroup_merge_table_holds():
    """200 distinct ids inside one tile: runs that find no free LDS entry go to the table directly"""
    ids = np.zeros((TH, TW), np.uint16)
    for k in range(200):
        y, x = (k // 50) * 4, (k % 50) * 5
        ids[y:y + 3, x:x + 4] = 24000 + 37 * k
    expected = check([ids])
    assert len(expected[0]) == 200 and all(row[5] == 12 and row[6] == 0 for row in expected[0])


def test_one_map_more_than_a_processing_batch():
    maps = [blob_map(40 + i, 24 + i, 37 + 2 * i, instances=5) for i in range(cs.BATCH + 1)]
    check(maps)


def test_blob_maps():
    assert_balanced(check(blob_maps(96, 160)))


def test_build_annotations_and_converter_device_equals_host(tmp_path):
    root = make_tree(str(tmp_path / "data"), variants=("plain",))
    gt = os.path.join(root, "gtFine")
    for kwargs in (dict(), dict(car_only=True), dict(drop_fragmented=False), dict(variant="foggy", beta=0.01)):
        assert cs.build_annotations(gt, "train", device="cuda", **kwargs) == cs.build_annotations(gt, "train", device="cpu", **kwargs)
    assert cs.build_annotations(gt, "train") == cs.build_annotations(gt, "train", device="cpu")     # default: the device
    convert = load_converter()
    name = "instancesonly_filtered_gtFine_train.json"
    for out, extra in ((str(tmp_path / "dev"), []), (str(tmp_path / "host"), ["--host"])):
        convert.main(["--datadir", root, "--outdir", out, "--splits", "train"] + extra)
    assert open(os.path.join(str(tmp_path / "dev"), name), "rb").read() == open(os.path.join(str(tmp_path / "host"), name), "rb").read()


def raw_tree(tmp_path):
    """four small maps in two cities with three kept instances each, plain and foggy images beside them"""
    from test_cityscapes_host import save_id_map, save_image

    root = str(tmp_path / "cityscapes")
    for k, (city, (H, W)) in enumerate([("aachen", (96, 192)), ("aachen", (96, 160)), ("bochum", (80, 192)), ("bochum", (96, 192))]):
        ids = np.full((H, W), 7, np.uint16)
        ids[10:50, 20 + 5 * k:70] = 26000 + k
        ids[30:75, 90:130 + 5 * k] = 24000 + k
        ids[60:78, 140:158] = 33000 + k
        stem = "%s_%06d_000019" % (city, k)
        save_id_map(os.path.join(root, "gtFine", "train", city, stem + "_gtFine_instanceIds.png"), ids)
        save_image(os.path.join(root, "leftImg8bit", "train", city, cs.image_name(stem)), H, W, k)
        save_image(os.path.join(root, "leftImg8bit_foggy", "train", city, cs.image_name(stem, "foggy")), H, W, 10 + k)
    return root


def test_training_starts_from_a_raw_tree(tmp_path):
    """tools/train_net_da.py --source cityscapes:ROOT,train --target cityscapes:ROOT,train,foggy: status 0, finite losses"""
    import re
    import subprocess
    import sys

    from test_cityscapes_host import ROOT

    root = raw_tree(tmp_path)
    out = str(tmp_path / "out")
    os.makedirs(out)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train_net_da.py"), "--config-file", os.path.join(
           ROOT, "configs/da_faster_rcnn/e2e_da_faster_rcnn_R_50_C4_cityscapes_to_foggy_cityscapes.yaml"),
           "--source", "cityscapes:%s,train" % root, "--target", "cityscapes:%s,train,foggy" % root,
           "SOLVER.MAX_ITER", "2", "SOLVER.CHECKPOINT_PERIOD", "0", "DATALOADER.NUM_WORKERS", "0",
           "INPUT.MIN_SIZE_TRAIN", "(96,)", "INPUT.MAX_SIZE_TRAIN", "192", "MODEL.OUTPUT_DIR", out, "MODEL.WEIGHT", ""]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    assert os.path.exists(os.path.join(out, "model_final.pth"))
    line = [ln for ln in res.stderr.splitlines() if "iter: 0 " in ln]
    assert line, res.stderr[-2000:]
    loss = re.search(r"loss: ([-+0-9.einfa]+)", line[0])
    assert loss and np.isfinite(float(loss.group(1))), line[0]


def test_score_net_evaluates_and_scores_a_raw_tree(tmp_path):
    """tools/score_net_da.py --dataset cityscapes:ROOT,train,foggy --config-file: the set's annotations written out, the
    evaluation pass of tools/test_net_da.py over them (seeded random weights), predictions under <ROOT's name>_<split and
    options>, then the COCO box AP table"""
    import subprocess
    import sys

    import torch

    from test_cityscapes_host import ROOT

    root = raw_tree(tmp_path)
    out = str(tmp_path / "out")
    os.makedirs(out)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "score_net_da.py"), "--dataset", "cityscapes:%s,train,foggy" % root,
           "--config-file", os.path.join(ROOT, "configs/da_faster_rcnn/e2e_da_faster_rcnn_R_50_C4_cityscapes_to_foggy_cityscapes.yaml"),
           "--output-dir", out, "DATALOADER.NUM_WORKERS", "0", "INPUT.MIN_SIZE_TEST", "96", "INPUT.MAX_SIZE_TEST", "192",
           "MODEL.WEIGHT", "", "MODEL.ROI_HEADS.SCORE_THRESH", "0.0"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    where = os.path.join(out, "inference", "cityscapes_train_foggy")
    predictions = torch.load(os.path.join(where, "predictions.pth"), weights_only=False)
    assert len(predictions) == 4
    assert "on 4 images" in res.stderr and "COCO box AP" in res.stderr
    assert os.path.exists(os.path.join(where, "coco_results.pth")) and os.path.exists(os.path.join(where, "bbox.json"))
    written = json.load(open(os.path.join(out, "cityscapes_train_foggy.json")))       # what tools/test_net_da.py evaluated
    assert written == cs.build_annotations(os.path.join(root, "gtFine"), "train", "foggy", device="cpu",
                                           image_dir=os.path.join(root, "leftImg8bit_foggy", "train"))


def test_full_size_map():
    """1024 x 2048, about 40 instances, against the host function and nothing more"""
    rng = np.random.RandomState(7)
    ids = rng.choice([7, 8, 11, 21, 23], size=(1024 // 64, 2048 // 64)).repeat(64, 0).repeat(64, 1).astype(np.uint16)
    yy, xx = np.mgrid[0:1024, 0:2048]
    for k in range(40):
        value = int(rng.choice([24, 25, 26, 27, 28, 31, 32, 33])) * 1000 + k
        cy, cx, h, w = int(rng.randint(300, 900)), int(rng.randint(0, 2048)), int(rng.randint(10, 300)), int(rng.randint(6, 400))
        if k % 2:
            ids[max(cy - h // 2, 0):cy + h // 2, max(cx - w // 2, 0):cx + w // 2] = value
        else:
            ids[((yy - cy) / (h / 2.0)) ** 2 + ((xx - cx) / (w / 2.0)) ** 2 <= 1.0] = value
        if k % 5 == 0:
            ids[int(rng.randint(0, 1024)), int(rng.randint(0, 2048))] = value
    expected = check([ids])
    assert len(expected[0]) >= 30 and 0 < sum(row[6] for row in expected[0]) < len(expected[0])
