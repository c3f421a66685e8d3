"""Raw Cityscapes datasets (da_detect_amd/data/cityscapes.py, tools/convert_cityscapes.py), host side.

The rules under test come from the reference's converters, which need cv2 and cityscapesscripts and cannot run here, so
nothing is recorded from them: the trees and maps are built below with numpy and Pillow, the expected values of the
closed-form cases are written out by hand, and `evaluate_map` is an independent statement of the rules — a boolean mask
per id, its extents and sum, and an explicit 8-connected flood fill for the component sizes.  It shares no code with
data/cityscapes.py (and needs no scipy)."""
import ctypes
import importlib.util
import json
import os
import re

import numpy as np
import pytest
import torch

from da_detect_amd import _lib
from da_detect_amd.data import cityscapes as cs
from da_detect_amd.data.build import _from_catalog, dataset_from_spec, parse_dataset_spec
from da_detect_amd.data.datasets import COCODataset

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ------------------------------------------------------------------------------------------ independent evaluator
def component_sizes(mask):
    """sizes of the 8-connected components of a boolean mask, by flood fill"""
    H, W = mask.shape
    seen = np.zeros((H, W), bool)
    sizes = []
    for y0 in range(H):
        for x0 in range(W):
            if not mask[y0, x0] or seen[y0, x0]:
                continue
            seen[y0, x0] = True
            stack, size = [(y0, x0)], 0
            while stack:
                y, x = stack.pop()
                size += 1
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        yy, xx = y + dy, x + dx
                        if 0 <= yy < H and 0 <= xx < W and mask[yy, xx] and not seen[yy, xx]:
                            seen[yy, xx] = True
                            stack.append((yy, xx))
            sizes.append(size)
    return sizes


def evaluate_map(ids):
    """-> [[id, x0, y0, x1, y1, pixelCount, fragmented]] for every id 24000 .. 33999 of the map, ascending"""
    rows = []
    for value in sorted(set(int(v) for v in np.asarray(ids).reshape(-1))):
        if value < 24000 or value > 33999:
            continue
        mask = np.asarray(ids) == value
        ys, xs = np.nonzero(mask)
        rows.append([value, int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()), int(mask.sum()),
                     int(min(component_sizes(mask)) <= 2)])
    return rows


def table(ids):
    return cs.instance_table_host(ids).tolist()


# --------------------------------------------------------------------------------------------------- random maps
def blob_map(seed, H, W, instances=12):
    """rectangles and discs 3 .. 40 pixels across on a background of ids < 1000 (stuff labels and a "group" region), later
    blobs covering earlier ones; 1- and 2-pixel fragments sprinkled onto about half of the instances"""
    rng = np.random.RandomState(seed)
    ids = rng.choice([0, 7, 8, 11, 21, 23, 26], size=(H // 8 + 1, W // 8 + 1)).repeat(8, 0).repeat(8, 1)[:H, :W].astype(np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    placed = []
    for k in range(instances):
        value = int(rng.choice([24, 25, 26, 27, 28, 29, 30, 31, 32, 33])) * 1000 + k
        size = int(rng.randint(3, 41))
        cy, cx = int(rng.randint(0, H)), int(rng.randint(0, W))
        if rng.randint(2):
            h = int(rng.randint(3, 41))
            ids[max(cy - h // 2, 0):cy + (h + 1) // 2, max(cx - size // 2, 0):cx + (size + 1) // 2] = value
        else:
            ids[(yy - cy) ** 2 + (xx - cx) ** 2 <= (size / 2.0) ** 2] = value
        placed.append(value)
    for value in placed:
        if rng.randint(2):
            continue
        for _ in range(int(rng.randint(1, 3))):
            y, x = int(rng.randint(0, H)), int(rng.randint(0, W))
            ids[y, x] = value
            if rng.randint(2):
                dy, dx = [(0, 1), (1, 0), (1, 1), (1, -1)][int(rng.randint(4))]
                if 0 <= y + dy < H and 0 <= x + dx < W:
                    ids[y + dy, x + dx] = value
    return ids


BLOB_SEEDS = tuple(range(8))


def blob_maps(H, W):
    return [blob_map(seed, H, W) for seed in BLOB_SEEDS]


def assert_balanced(tables):
    """both outcomes of the fragment rule are well represented"""
    flags = [row[6] for t in tables for row in t]
    assert len(flags) >= 40
    assert sum(flags) * 4 >= len(flags), "fewer than a quarter of the instances are fragmented"
    assert (len(flags) - sum(flags)) * 4 >= len(flags), "fewer than a quarter of the instances are whole"


# --------------------------------------------------------------------------------------------------- tiny trees
def save_id_map(path, ids):
    from PIL import Image

    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(np.asarray(ids).astype(np.uint16)).save(path)


def save_image(path, H, W, seed=0):
    from PIL import Image

    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(np.random.RandomState(seed).randint(0, 256, (H, W, 3)).astype(np.uint8)).save(path)


def tree_maps():
    """{(city, stem): id map}: two cities, different sizes, one map without any instance"""
    a = np.full((20, 30), 7, np.int64)
    a[2:6, 3:9] = 26001          # car  x 3..8  y 2..5  24 px
    a[10:13, 20:22] = 24000      # person x 20..21 y 10..12 6 px
    a[15, 5] = 26003             # single pixel: dropped
    a[8:12, 12:16] = 29001       # caravan: not kept
    b = np.full((16, 24), 8, np.int64)      # no instance at all
    c = np.full((18, 18), 11, np.int64)
    c[0:3, 0:3] = 33999          # bicycle
    c[5:9, 5:9] = 25002          # rider
    c[5:9, 10:14] = 26 * 1000 + 7
    c[16, 16] = 26               # group of cars: ignored
    return {("aachen", "aachen_000001_000019"): a, ("aachen", "aachen_000000_000019"): b,
            ("bochum", "bochum_000000_000313"): c}


def make_tree(root, split="train", per_city=True, variants=("plain",), betas=(0.02,)):
    for (city, stem), ids in tree_maps().items():
        save_id_map(os.path.join(root, "gtFine", split, city, stem + "_gtFine_instanceIds.png"), ids)
        for variant in variants:
            names = [cs.image_name(stem, variant, b) for b in (betas if variant == "foggy" else (0.02,))]
            for name in names:
                folder = os.path.join(root, cs.IMAGE_DIRS[variant], split, city if per_city else "")
                save_image(os.path.join(folder, name), ids.shape[0], ids.shape[1])
    return root


# --------------------------------------------------------------------------------------------- closed-form cases
def test_touches_all_four_borders():
    ids = np.zeros((6, 9), np.int64)
    ids[:, 4] = 26005
    ids[2, :] = 26005
    assert table(ids) == [[26005, 0, 0, 8, 5, 6 + 9 - 1, 0]]


def test_single_pixel_is_fragmented():
    ids = np.zeros((5, 5), np.int64)
    ids[2, 3] = 24001
    assert table(ids) == [[24001, 3, 2, 3, 2, 1, 1]]


def test_diagonal_pair_is_fragmented():
    ids = np.zeros((5, 5), np.int64)
    ids[1, 1] = ids[2, 2] = 25001
    assert table(ids) == [[25001, 1, 1, 2, 2, 2, 1]]


def test_three_pixel_l_is_kept():
    ids = np.zeros((5, 5), np.int64)
    ids[1, 1] = ids[2, 1] = ids[2, 2] = 27001
    assert table(ids) == [[27001, 1, 1, 2, 2, 3, 0]]
    line = np.zeros((3, 7), np.int64)
    line[1, 2:5] = 27002                     # a 3-pixel line: its ends have one neighbour, the middle has two
    assert table(line) == [[27002, 2, 1, 4, 1, 3, 0]]


def test_body_with_stray_fragment(tmp_path):
    ids = np.full((12, 16), 7, np.int64)
    ids[2:8, 3:9] = 26001
    ids[10, 14] = 26001
    assert table(ids) == [[26001, 3, 2, 14, 10, 37, 1]]
    save_id_map(str(tmp_path / "gtFine" / "val" / "ulm" / "ulm_0_0_gtFine_instanceIds.png"), ids)
    kept = cs.build_annotations(str(tmp_path / "gtFine"), "val", drop_fragmented=False, device="cpu")
    assert [a["bbox"] for a in kept["annotations"]] == [[3, 2, 12, 9]] and kept["annotations"][0]["area"] == 37
    dropped = cs.build_annotations(str(tmp_path / "gtFine"), "val", device="cpu")
    assert dropped["annotations"] == [] and len(dropped["images"]) == 1


def test_id_and_class_edges(tmp_path):
    ids = np.zeros((8, 40), np.int64)
    for k, value in enumerate((999, 23999, 26, 34000, 24000, 33999, 29001, 30001, 26123)):
        ids[2:5, 4 * k:4 * k + 3] = value
    assert [row[0] for row in table(ids)] == [24000, 26123, 29001, 30001, 33999]
    assert table(ids) == evaluate_map(ids)
    save_id_map(str(tmp_path / "gtFine" / "val" / "ulm" / "ulm_0_0_gtFine_instanceIds.png"), ids)
    full = cs.build_annotations(str(tmp_path / "gtFine"), "val", device="cpu")
    assert [c["name"] for c in full["categories"]] == ["person", "rider", "car", "truck", "bus", "train", "motorcycle", "bicycle"]
    assert [c["id"] for c in full["categories"]] == list(range(1, 9))
    assert [(a["category_id"], a["bbox"]) for a in full["annotations"]] == [(1, [16, 2, 3, 3]), (3, [32, 2, 3, 3]),
                                                                             (8, [20, 2, 3, 3])]
    car = cs.build_annotations(str(tmp_path / "gtFine"), "val", car_only=True, device="cpu")
    assert car["categories"] == [{"id": 1, "name": "car"}]
    assert [(a["category_id"], a["bbox"], a["area"], a["iscrowd"]) for a in car["annotations"]] == [(1, [32, 2, 3, 3], 9, 0)]


def test_host_table_equals_evaluator_on_blob_maps():
    maps = blob_maps(64, 96)
    tables = [table(m) for m in maps]
    for m, t in zip(maps, tables):
        assert t == evaluate_map(m)
    assert_balanced(tables)


def test_host_table_dtypes_and_empty():
    out = cs.instance_table_host(np.zeros((3, 4), np.uint16))
    assert out.shape == (0, 7) and out.dtype == np.int32
    ids = blob_map(1, 40, 40)
    for dtype in (np.uint16, np.int32, np.int64):
        assert cs.instance_table_host(ids.astype(dtype)).tolist() == table(ids)


# ------------------------------------------------------------------------------------------- build_annotations
@pytest.mark.parametrize("variant", ["plain", "foggy", "rain"])
def test_build_annotations_on_a_two_city_tree(tmp_path, variant):
    root = make_tree(str(tmp_path), variants=(variant,))
    data = cs.build_annotations(os.path.join(root, "gtFine"), "train", variant,
                                image_dir=os.path.join(root, cs.IMAGE_DIRS[variant], "train"), device="cpu")
    tail = "_leftImg8bit_foggy_beta_0.02.png" if variant == "foggy" else "_leftImg8bit.png"
    assert [im["file_name"] for im in data["images"]] == [
        "aachen/aachen_000000_000019" + tail, "aachen/aachen_000001_000019" + tail, "bochum/bochum_000000_000313" + tail]
    assert [im["id"] for im in data["images"]] == [0, 1, 2]
    assert [(im["height"], im["width"]) for im in data["images"]] == [(16, 24), (20, 30), (18, 18)]
    assert "segmentation" not in data["annotations"][0]
    got = [(a["id"], a["image_id"], a["category_id"], a["bbox"], a["area"], a["iscrowd"]) for a in data["annotations"]]
    assert got == [(0, 1, 1, [20, 10, 2, 3], 6, 0), (1, 1, 3, [3, 2, 6, 4], 24, 0),             # ascending id: 24000, 26001
                   (2, 2, 2, [5, 5, 4, 4], 16, 0), (3, 2, 3, [10, 5, 4, 4], 16, 0), (4, 2, 8, [0, 0, 3, 3], 9, 0)]
    assert not [a for a in data["annotations"] if a["image_id"] == 0]      # no instance, yet an `images` entry


def test_file_names_flat_and_per_city_and_betas(tmp_path):
    flat = make_tree(str(tmp_path / "flat"), per_city=False, variants=("plain", "foggy"), betas=(0.02, 0.01, 0.005))
    names = [im["file_name"] for im in cs.build_annotations(os.path.join(flat, "gtFine"), "train", device="cpu",
                                                            image_dir=os.path.join(flat, "leftImg8bit", "train"))["images"]]
    assert names == ["aachen_000000_000019_leftImg8bit.png", "aachen_000001_000019_leftImg8bit.png",
                     "bochum_000000_000313_leftImg8bit.png"]
    no_dir = cs.build_annotations(os.path.join(flat, "gtFine"), "train", device="cpu")
    assert [im["file_name"] for im in no_dir["images"]] == names
    for beta, text in ((0.02, "0.02"), (0.01, "0.01"), (0.005, "0.005")):
        data = cs.build_annotations(os.path.join(flat, "gtFine"), "train", "foggy", beta, device="cpu",
                                    image_dir=os.path.join(flat, "leftImg8bit_foggy", "train"))
        assert data["images"][0]["file_name"] == "aachen_000000_000019_leftImg8bit_foggy_beta_%s.png" % text
        for im in data["images"]:
            assert os.path.exists(os.path.join(flat, "leftImg8bit_foggy", "train", im["file_name"]))
    with pytest.raises(ValueError):
        cs.build_annotations(os.path.join(flat, "gtFine"), "train", "foggy", 0.03, device="cpu")
    with pytest.raises(ValueError):
        cs.build_annotations(os.path.join(flat, "gtFine"), "train", "snow", device="cpu")


def test_mode_i_maps_and_ids_beyond_16_bits(tmp_path):
    from PIL import Image

    ids = np.full((6, 8), 7, np.int32)
    ids[1:4, 2:6] = 26001
    folder = tmp_path / "gtFine" / "val" / "ulm"
    os.makedirs(str(folder))
    path = str(folder / "ulm_0_0_gtFine_instanceIds.png")
    Image.fromarray(ids).save(path, format="TIFF")               # mode I, 32 bits per pixel (Pillow reads by content)
    assert Image.open(path).mode == "I"
    assert cs.read_id_map(path).dtype == np.uint16
    data = cs.build_annotations(str(tmp_path / "gtFine"), "val", device="cpu")
    assert [a["bbox"] for a in data["annotations"]] == [[2, 1, 4, 3]]
    ids[0, 0] = 65536
    Image.fromarray(ids).save(path, format="TIFF")
    with pytest.raises(ValueError) as err:
        cs.build_annotations(str(tmp_path / "gtFine"), "val", device="cpu")
    assert "ulm_0_0_gtFine_instanceIds.png" in str(err.value)
    Image.fromarray(np.full((6, 8), 26, np.uint8)).save(path, format="PNG")      # 8 bits: a labelIds map, not an id map
    with pytest.raises(ValueError) as err:
        cs.read_id_map(path)
    assert "ulm_0_0_gtFine_instanceIds.png" in str(err.value)


# ------------------------------------------------------------------------------------ dataset and spec surface
def load_converter():
    spec = importlib.util.spec_from_file_location("convert_cityscapes", os.path.join(ROOT, "tools", "convert_cityscapes.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def same_samples(a, b):
    assert len(a) == len(b) > 0
    for i in range(len(a)):
        (img_a, tgt_a, _), (img_b, tgt_b, _) = a[i], b[i]
        assert img_a.size == img_b.size and np.array_equal(np.asarray(img_a), np.asarray(img_b))
        assert torch.equal(tgt_a.bbox, tgt_b.bbox)
        for field in ("labels", "is_source"):
            assert torch.equal(tgt_a.get_field(field), tgt_b.get_field(field))
        assert a.get_img_info(i) == b.get_img_info(i)


def test_dataset_equals_cocodataset_over_the_converted_json(tmp_path):
    root = make_tree(str(tmp_path / "data"), variants=("plain", "foggy"))
    out = str(tmp_path / "annotations")
    convert = load_converter()
    convert.main(["--datadir", root, "--outdir", out, "--dataset", "cityscapes_instance_only", "--splits", "train", "--host"])
    convert.main(["--datadir", root, "--outdir", out, "--dataset", "foggy_cityscapes", "--splits", "train", "--host"])
    plain = cs.CityscapesDataset(root, "train", device="cpu")
    same_samples(plain, COCODataset(os.path.join(out, "instancesonly_filtered_gtFine_train.json"),
                                    os.path.join(root, "leftImg8bit", "train"), False))
    assert torch.equal(plain[1][1].bbox, torch.tensor([[20., 10., 21., 12.], [3., 2., 8., 5.]]))
    assert plain[1][1].get_field("labels").tolist() == [1, 3] and plain[1][1].get_field("is_source").all()
    foggy = cs.CityscapesDataset(root, "train", "foggy", is_source=False, device="cpu")
    same_samples(foggy, COCODataset(os.path.join(out, "foggy_instancesonly_filtered_gtFine_train.json"),
                                    os.path.join(root, "leftImg8bit_foggy", "train"), False, is_source=False))
    assert not foggy[1][1].get_field("is_source").any()
    assert len(cs.CityscapesDataset(root, "train", remove_images_without_annotations=True, device="cpu")) == 2
    pair = cs.write_annotation_file(root, "train,foggy", str(tmp_path / "set.json"), device="cpu")      # what score_net_da.py hands on
    assert pair == (str(tmp_path / "set.json"), os.path.join(root, "leftImg8bit_foggy", "train"))
    assert open(pair[0]).read() == open(os.path.join(out, "foggy_instancesonly_filtered_gtFine_train.json")).read()
    assert plain.map_class_id_to_class_name(3) == "car" and plain.get_groundtruth(2).get_field("labels").tolist() == [2, 3, 8]


def test_spec_forms(tmp_path):
    assert parse_dataset_spec("ann.json,imgs") == ("ann.json", "imgs")
    assert parse_dataset_spec("voc:/d/VOC2007,test") == ("voc:/d/VOC2007", "test")
    assert parse_dataset_spec("rain:/masks") == ("rain:/masks", "")
    assert parse_dataset_spec("cityscapes:/d/cs,train") == ("cityscapes:/d/cs", "train")
    assert parse_dataset_spec("cityscapes:/d/cs,val,foggy=0.01,caronly") == ("cityscapes:/d/cs", "val,foggy=0.01,caronly")
    assert cs.parse_options("train") == dict(split="train", variant="plain", beta=0.02, car_only=False)
    assert cs.parse_options("val,foggy") == dict(split="val", variant="foggy", beta=0.02, car_only=False)
    assert cs.parse_options("val,foggy=0.005") == dict(split="val", variant="foggy", beta=0.005, car_only=False)
    assert cs.parse_options("train,rain,caronly") == dict(split="train", variant="rain", beta=0.02, car_only=True)
    assert cs.parse_options("train,caronly") == dict(split="train", variant="plain", beta=0.02, car_only=True)
    for bad in ("cityscapes:/d/cs", "cityscapes:/d/cs,train,snow", "cityscapes:/d/cs,train,foggy=0.5",
                "cityscapes:/d/cs,train,foggy,rain"):
        with pytest.raises(ValueError):
            parse_dataset_spec(bad)
    root = make_tree(str(tmp_path), variants=("plain", "foggy"), betas=(0.01,))
    source = dataset_from_spec(("cityscapes:" + root, "train"), None, is_train=True, is_source=True, device="cpu")
    assert isinstance(source, cs.CityscapesDataset) and len(source) == 2            # training drops the empty image
    target = dataset_from_spec(parse_dataset_spec("cityscapes:%s,train,foggy=0.01,caronly" % root), None, False, False,
                               decode_to_tensor=True, device="cpu")
    assert len(target) == 3 and target.variant == "foggy" and target.car_only
    pixels, boxes, _ = target[1]
    assert pixels.dtype == torch.uint8 and tuple(pixels.shape) == (20, 30, 3)
    assert boxes.get_field("labels").tolist() == [1] and not boxes.get_field("is_source").any()


def test_tools_accept_the_spec():
    for tool in ("train_net_da", "score_net_da"):        # (tools/test_net_da.py stays as it is: score_net_da.py runs the pass)
        spec = importlib.util.spec_from_file_location(tool, os.path.join(ROOT, "tools", tool + ".py"))
        module = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(module)
        assert module._pair("cityscapes:/d/cs,val,foggy=0.01,caronly") == ("cityscapes:/d/cs", "val,foggy=0.01,caronly"), tool
        assert module._pair("cityscapes:/d/cs,train") == ("cityscapes:/d/cs", "train"), tool
        assert module._pair("ann.json,imgs") == ("ann.json", "imgs"), tool
        with pytest.raises(ValueError):
            module._pair("cityscapes:/d/cs,train,snow")
    spec = importlib.util.spec_from_file_location("score_net_da", os.path.join(ROOT, "tools", "score_net_da.py"))
    score = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(score)
    assert score._set_name(("cityscapes:/d/cs/", "val,foggy=0.01")) == "cs_val_foggy=0.01"
    assert score._set_name(("voc:/d/VOC2007", "test")) == "VOC2007_test" and score._set_name(("/a/b/ann.json", "imgs")) == "ann"


def test_register_cityscapes_resolves(tmp_path):
    from da_detect_amd.config.paths_catalog import DatasetCatalog

    root = make_tree(str(tmp_path), split="val", variants=("rain",))
    name = "cityscapes_raw_rain_val"
    DatasetCatalog.register_cityscapes(name, root, "val", variant="rain", car_only=True, device="cpu")
    try:
        entry = DatasetCatalog.get(name)
        assert entry["factory"] == "CityscapesDataset"
        assert entry["args"] == dict(root=root, split="val", variant="rain", beta=0.02, car_only=True, device="cpu")
        dataset = _from_catalog(name, DatasetCatalog, None, False, False)
        assert isinstance(dataset, cs.CityscapesDataset) and len(dataset) == 3
        assert dataset[2][1].get_field("labels").tolist() == [1]
        assert dataset.root == os.path.join(root, "leftImg8bit_rain", "val")
        with pytest.raises(ValueError):
            DatasetCatalog.register_cityscapes("x", root, "val", variant="snow")
    finally:
        DatasetCatalog.DATASETS.pop(name, None)


# ------------------------------------------------------------------------------------------- converter and ABI
def test_converter_writes_the_reference_file_names(tmp_path):
    root = make_tree(str(tmp_path / "data"), split="train")
    make_tree(root, split="val")
    out = str(tmp_path / "out")
    convert = load_converter()
    for dataset, pattern in (("cityscapes_instance_only", "instancesonly_filtered_gtFine_%s.json"),
                             ("foggy_cityscapes", "foggy_instancesonly_filtered_gtFine_%s.json"),
                             ("cityscapes_car_only", "caronly_filtered_gtFine_%s.json")):
        convert.main(["--datadir", root, "--outdir", out, "--dataset", dataset, "--host"])
        for split in ("train", "val"):
            data = json.load(open(os.path.join(out, pattern % split)))
            assert sorted(data) == ["annotations", "categories", "images"] and len(data["images"]) == 3
            assert len(data["annotations"]) == (2 if dataset == "cityscapes_car_only" else 5)
    foggy = json.load(open(os.path.join(out, "foggy_instancesonly_filtered_gtFine_val.json")))
    assert foggy["images"][0]["file_name"].endswith("_leftImg8bit_foggy_beta_0.02.png")
    convert.main(["--datadir", root, "--outdir", out, "--splits", "val", "--host", "--keep-fragmented"])
    assert len(json.load(open(os.path.join(out, "instancesonly_filtered_gtFine_val.json")))["annotations"]) == 6


def test_instance_boxes_symbols_and_constants():
    header = open(os.path.join(ROOT, "include", "dadet.h")).read()
    for name, n_args in (("dadet_instance_boxes", 10), ("dadet_instance_boxes_workspace_bytes", 2)):
        proto = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert proto, "include/dadet.h does not declare %s" % name
        assert len(proto.group(1).split(",")) == len(_lib._SIGNATURES[name]) == n_args
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert "instance_boxes.hip" in open(os.path.join(ROOT, "da_detect_amd", "csrc", "Makefile")).read()
    for macro, value in (("MAX_BATCH", cs.MAX_BATCH), ("MAX_SIDE", cs.MAX_SIDE), ("FIRST_ID", cs.FIRST_ID), ("SLOTS", cs.SLOTS),
                         ("COLUMNS", cs.COLUMNS), ("TILE_W", cs.TILE_W), ("TILE_H", cs.TILE_H), ("SEGMENT", cs.SEGMENT)):
        found = re.search(r"#define\s+DADET_INSTANCE_BOXES_%s\s+(\d+)" % macro, header)
        assert found and int(found.group(1)) == value, macro
    assert cs.BATCH <= cs.MAX_BATCH
