"""Shared by tests/test_overlay_host.py and tests/test_overlay_gpu.py: the drawing rule of engine/overlay.py stated once more,
pixel by pixel and straight from its wording (so the slicing renderer is not its own judge), random draw lists, and the
four-image COCO-format set the tool tests draw."""
import importlib.util
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reference_render(image, records):
    """DESIGN.md 3j read literally: for every pixel, pass A over the records in order, then pass B"""
    from da_detect_amd.engine import _glyphs

    img = np.array(image, dtype=np.uint8)
    H, W = img.shape[:2]
    for y in range(H):
        for x in range(W):
            v = [int(t) for t in img[y, x]]
            for r in records:
                if not (r.x0 <= x <= r.x1 and r.y0 <= y <= r.y1):
                    continue
                if r.a > 0:
                    v = [(c * r.a + t * (256 - r.a) + 128) >> 8 for c, t in zip(r.color, v)]
                if x - r.x0 < r.w or r.x1 - x < r.w or y - r.y0 < r.w or r.y1 - y < r.w:
                    v = list(r.color)
            for r in records:
                n = len(r.label)
                if n == 0 or not (r.tx - 1 <= x <= r.tx + 6 * n and r.ty - 1 <= y <= r.ty + 11):
                    continue
                v = list(r.color)
                dx, dy = x - r.tx, y - r.ty
                if 0 <= dx < 6 * n and 0 <= dy < 11:
                    bits = int(_glyphs.GLYPHS[ord(r.label[dx // 6]) - 0x20, dy])
                    if (bits >> (5 - dx % 6)) & 1:
                        red, green, blue = r.color
                        dark = (red * 19595 + green * 38470 + blue * 7471 + 0x8000) >> 16 < 128
                        v = [255] * 3 if dark else [0] * 3
            img[y, x] = v
    return img


def background(rng, H, W):
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


_ALPHABET = "".join(chr(c) for c in range(0x20, 0x7f))


def random_label(rng, n):
    return "".join(_ALPHABET[int(i)] for i in rng.integers(0, len(_ALPHABET), n))


def random_records(rng, n, H, W, alphas=(0, 0, 64, 128, 256), max_label=8, margin=10):
    """n records with corners in [-margin, size + margin), distinct colours, labels of 0 .. max_label characters"""
    from da_detect_amd.engine.overlay import make_record

    out = []
    for k in range(n):
        xs = np.sort(rng.integers(-margin, W + margin, 2))
        ys = np.sort(rng.integers(-margin, H + margin, 2))
        color = ((37 * k + 11) % 256, (91 * k + 5) % 256, (53 * k + 200) % 256)
        out.append(make_record((xs[0], ys[0], xs[1], ys[1]), color, random_label(rng, int(rng.integers(0, max_label + 1))),
                               thickness=int(rng.integers(1, 6)), fill_alpha=int(alphas[int(rng.integers(0, len(alphas)))])))
    return out


# --------------------------------------------------------------------------------------------------------- the tool's set
SET_SIZES = ((40, 70), (33, 65), (50, 50), (16, 130))          # (H, W) of the four images
SET_NAMES = ("person", "car", "bus")


def write_coco_set(folder):
    """four random PNG images, a COCO-format annotation file with three categories, and two prediction files (one BoxList
    per image, at another size than the image so the tool's resize shows) -> dict of paths"""
    import torch
    from PIL import Image

    from da_detect_amd.structures.bounding_box import BoxList

    folder = str(folder)
    rng = np.random.default_rng(77)
    os.makedirs(os.path.join(folder, "img"), exist_ok=True)
    images, annotations = [], []
    for i, (H, W) in enumerate(SET_SIZES):
        name = "frame_%d.png" % i
        Image.fromarray(background(rng, H, W)).save(os.path.join(folder, "img", name))
        images.append({"id": 100 + i, "file_name": name, "height": H, "width": W})
        for k in range(2):
            x, y = int(rng.integers(0, W // 2)), int(rng.integers(0, H // 2))
            annotations.append({"id": len(annotations) + 1, "image_id": 100 + i, "category_id": (5, 7, 9)[(i + k) % 3],
                                "bbox": [x, y, int(rng.integers(6, W // 2)), int(rng.integers(6, H // 2))], "iscrowd": 0,
                                "area": 1.0})
    ann = os.path.join(folder, "ann.json")
    with open(ann, "w") as f:
        json.dump({"images": images, "annotations": annotations,
                   "categories": [{"id": c, "name": n} for c, n in zip((5, 7, 9), SET_NAMES)]}, f)
    paths = {"ann": ann, "img": os.path.join(folder, "img"), "spec": "%s,%s" % (ann, os.path.join(folder, "img"))}
    for which in ("a", "b"):
        predictions = []
        for i, (H, W) in enumerate(SET_SIZES):
            n = 0 if (which == "b" and i == 2) else 5
            xy = rng.uniform(-8, (2 * W * 0.6, 2 * H * 0.6), (n, 2))
            boxes = np.concatenate([xy, xy + rng.uniform(3, (2 * W * 0.5, 2 * H * 0.5), (n, 2))], 1).astype(np.float32)
            p = BoxList(torch.from_numpy(boxes), (2 * W, 2 * H), mode="xyxy")
            p.add_field("labels", torch.from_numpy(rng.integers(1, 4, n)))
            p.add_field("scores", torch.from_numpy(rng.uniform(0.5, 1.0, n).astype(np.float32)))
            predictions.append(p)
        paths[which] = os.path.join(folder, "predictions_%s.pth" % which)
        torch.save(predictions, paths[which])
    return paths


def load_tool():
    spec = importlib.util.spec_from_file_location("draw_detections", os.path.join(ROOT, "tools", "draw_detections.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def expected_panels(paths, index, gt, prediction_files, threshold=0.7, **style):
    """what the tool must write for image `index`: render_host panels of the original image, stacked top to bottom"""
    import torch
    from PIL import Image

    from da_detect_amd.data.datasets import COCODataset
    from da_detect_amd.engine import overlay

    dataset = COCODataset(paths["ann"], paths["img"], False)
    H, W = SET_SIZES[index]
    pixels = np.array(Image.open(os.path.join(paths["img"], "frame_%d.png" % index)).convert("RGB"))
    names = [""] + list(SET_NAMES)
    panels = []
    if gt:
        target = dataset[index][1]
        panels.append(overlay.render_host(pixels, overlay.build_draw_list(target.copy_with_fields(["labels"]), names, **style)))
    for path in prediction_files:
        p = torch.load(path, weights_only=False)[index].resize((W, H))
        top = overlay.select_top_predictions(p, threshold)
        panels.append(overlay.render_host(pixels, overlay.build_draw_list(top, names, **style)))
    return np.concatenate(panels, axis=0)
