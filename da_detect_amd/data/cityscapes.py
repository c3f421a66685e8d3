"""Raw Cityscapes as a dataset: COCO-style box annotations straight from the `*_gtFine_instanceIds.png` maps (reference:
tools/cityscapes/convert_cityscapes_to_coco.py:130-271, convert_foggy_cityscapes_to_coco.py, convert_cityscapes_to_caronly_coco.py
and instances2dict_with_polygons.py:27-78, which need cv2, cityscapesscripts, h5py and scipy.misc).  The rules, per id map:

  * ids >= 1000 are instances of label id // 1000; eight labels are kept, as categories 1 .. 8 in this order: person 24,
    rider 25, car 26, truck 27, bus 28, train 31, motorcycle 32, bicycle 33 (car-only: car alone, as category 1);
  * bbox = [x0, y0, x1 - x0 + 1, y1 - y0 + 1] over ALL pixels carrying the id, area = their number, iscrowd = 0;
  * an instance is dropped whole when one of its 8-connected components has at most 2 pixels (the reference's "invalid
    contours": a contour of <= 2 points) — `fragmented` below, a 5 x 5 stencil: with n(p) the number of same-id
    8-neighbours of p, p lies in such a component iff n(p) == 0, or n(p) == 1 and its one neighbour q has n(q) == 1;
  * one `images` entry per id map, sorted by path, the size taken from the map; annotations in ascending instance id.

`instance_table_host` states this in numpy; `instance_table_device` computes the same table for a batch of maps with
csrc/instance_boxes.hip.  Filtering by class and by `fragmented` happens here, on the host, from the full table.
DESIGN.md section 3h."""
import ctypes
import json
import os
import time

import numpy as np

from .datasets import COCODataset

FIRST_ID, SLOTS, COLUMNS = 24000, 10000, 7      # DADET_INSTANCE_BOXES_FIRST_ID / _SLOTS / _COLUMNS
MAX_BATCH = 32                                  # DADET_INSTANCE_BOXES_MAX_BATCH
MAX_SIDE = 32767                                # DADET_INSTANCE_BOXES_MAX_SIDE
TILE_W, TILE_H, SEGMENT = 256, 16, 64           # DADET_INSTANCE_BOXES_TILE_W / _TILE_H / _SEGMENT (csrc/instance_boxes.hip)
BATCH = 16                                      # maps per launch sequence of a split

CATEGORIES = ("person", "rider", "car", "truck", "bus", "train", "motorcycle", "bicycle")
LABEL_IDS = {"person": 24, "rider": 25, "car": 26, "truck": 27, "bus": 28, "train": 31, "motorcycle": 32, "bicycle": 33}
VARIANTS = ("plain", "foggy", "rain")
BETAS = (0.02, 0.01, 0.005)
IMAGE_DIRS = {"plain": "leftImg8bit", "foggy": "leftImg8bit_foggy", "rain": "leftImg8bit_rain"}
ID_SUFFIX = "_gtFine_instanceIds.png"
PREFIX = "cityscapes:"


# ------------------------------------------------------------------------------------------------------- the table
def _shift(a, dy, dx, fill):
    """out[y, x] = a[y + dy, x + dx], `fill` where that lies beyond the map"""
    H, W = a.shape
    out = np.full_like(a, fill)
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    out[yd, xd] = a[ys, xs]
    return out


def instance_table_host(ids):
    """one id map [H, W] (any integer dtype) -> int32 [k, 7] rows [id, x0, y0, x1, y1, pixelCount, fragmented], one per id
    24000 .. 33999 present, in ascending id; the box is the inclusive extent of all pixels carrying the id"""
    ids = np.asarray(ids)
    assert ids.ndim == 2
    ids = ids.astype(np.int64)
    inst = (ids >= FIRST_ID) & (ids < FIRST_ID + SLOTS)
    if not inst.any():
        return np.zeros((0, COLUMNS), np.int32)
    steps = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)]
    same = [inst & (_shift(ids, dy, dx, -1) == ids) for dy, dx in steps]
    n = np.sum(same, axis=0, dtype=np.int64)
    lone_neighbour = np.zeros(ids.shape, bool)           # some same-id neighbour q has n(q) == 1
    for (dy, dx), s in zip(steps, same):
        lone_neighbour |= s & (_shift(n, dy, dx, 0) == 1)
    small = inst & ((n == 0) | ((n == 1) & lone_neighbour))
    ys, xs = np.nonzero(inst)
    order = np.argsort(ids[ys, xs], kind="stable")
    ys, xs = ys[order], xs[order]
    uniq, first, counts = np.unique(ids[ys, xs], return_index=True, return_counts=True)
    rows = np.stack([uniq, np.minimum.reduceat(xs, first), np.minimum.reduceat(ys, first), np.maximum.reduceat(xs, first),
                     np.maximum.reduceat(ys, first), counts,
                     np.maximum.reduceat(small[ys, xs].astype(np.int64), first)], axis=1)
    return rows.astype(np.int32)


def workspace_bytes(n):
    from .. import _lib

    out = ctypes.c_size_t(0)
    _lib.call("dadet_instance_boxes_workspace_bytes", int(n), ctypes.byref(out))
    return int(out.value)


def _as_uint16(m, name="id map"):
    m = np.asarray(m)
    if m.ndim != 2 or m.size == 0 or m.dtype.kind not in "iub":
        raise ValueError("%s: an id map is a non-empty 2-D integer array" % name)
    if m.dtype != np.uint16:
        if m.min() < 0 or m.max() > 65535:
            raise ValueError("%s: instance ids must fit 16 bits (found %d .. %d)" % (name, int(m.min()), int(m.max())))
        m = m.astype(np.uint16)
    return m


class DeviceTables(object):
    """the buffers of the device path, kept across the batches of a split: a pinned staging buffer for the packed maps
    (allocated pinned and filled in place; it grows to the largest batch seen), the device copy, workspace, rows and counts,
    and pinned buffers the result comes back into.  `tables(maps)`: <= MAX_BATCH uint16 maps -> their tables with one
    upload, one launch sequence and one host wait; the buffers are free again when it returns."""

    def __init__(self, device="cuda"):
        import torch

        from .. import _lib

        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.DadetError("instance tables on the device: %s is no HIP device" % device)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        self.staging = self.ids = None               # int16: the 16 bits of every pixel under torch's signed type
        self.n = 0                                   # maps the result buffers hold

    def _reserve(self, total, n):
        import torch

        if self.staging is None or self.staging.numel() < total:
            self.staging = torch.empty(total, dtype=torch.int16, pin_memory=True)
            self.ids = torch.empty(total, dtype=torch.int16, device=self.device)
        if self.n < n:
            self.work = torch.empty(workspace_bytes(n), dtype=torch.uint8, device=self.device)
            self.rows = torch.empty((n, SLOTS, COLUMNS), dtype=torch.int32, device=self.device)
            self.counts = torch.empty(n, dtype=torch.int32, device=self.device)
            self.rows_host = torch.empty((n, SLOTS, COLUMNS), dtype=torch.int32, pin_memory=True)
            self.counts_host = torch.empty(n, dtype=torch.int32, pin_memory=True)
            self.n = n

    def tables(self, maps):
        import torch

        from .. import _lib

        n = len(maps)
        assert 1 <= n <= MAX_BATCH
        sizes = [m.size for m in maps]
        offsets = np.zeros(n, np.int64)
        offsets[1:] = np.cumsum(sizes)[:-1]
        total = int(sum(sizes))
        with torch.cuda.device(self.device):
            self._reserve(total, n)
            flat = self.staging.numpy().view(np.uint16)
            for m, o in zip(maps, offsets):
                assert m.dtype == np.uint16
                flat[o:o + m.size] = m.reshape(-1)
            stream = torch.cuda.current_stream(self.device)
            self.ids[:total].copy_(self.staging[:total], non_blocking=True)
            hw = np.ascontiguousarray([[m.shape[0], m.shape[1]] for m in maps], dtype=np.int32)
            _lib.call("dadet_instance_boxes", ctypes.c_void_p(self.ids.data_ptr()), total,
                      hw.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), n,
                      ctypes.c_void_p(self.rows.data_ptr()), ctypes.c_void_p(self.counts.data_ptr()),
                      ctypes.c_void_p(self.work.data_ptr()), int(self.work.numel()), ctypes.c_void_p(stream.cuda_stream))
            self.rows_host[:n].copy_(self.rows[:n], non_blocking=True)
            self.counts_host[:n].copy_(self.counts[:n], non_blocking=True)
            stream.synchronize()                          # the batch's one host wait
        return [self.rows_host[i, :int(self.counts_host[i])].numpy().copy() for i in range(n)]


def instance_table_device(list_of_maps, device="cuda", buffers=None):
    """`instance_table_host` of every map of the list, on the HIP device: maps of any mix of sizes, processed BATCH at a time.
    buffers: a DeviceTables to reuse (a split is converted with one)"""
    buffers = DeviceTables(device) if buffers is None else buffers
    maps = [_as_uint16(m, "map %d" % i) for i, m in enumerate(list_of_maps)]
    out = []
    for at in range(0, len(maps), BATCH):
        out.extend(buffers.tables(maps[at:at + BATCH]))
    return out

# ------------------------------------------------------------------------------------------------- annotations
def device_available():
    """a HIP device is visible and the library is built"""
    import torch

    from .. import _lib

    return bool(torch.cuda.is_available()) and os.path.exists(_lib.LIB_PATH)


def list_id_maps(gt_dir, split):
    """the `*_gtFine_instanceIds.png` files under gt_dir/split, sorted by path -> [(city or "", stem, path)]"""
    top = os.path.join(gt_dir, split)
    if not os.path.isdir(top):
        raise ValueError("no directory %s" % top)
    found = []
    for folder, _, files in os.walk(top):
        for f in files:
            if f.endswith(ID_SUFFIX):
                found.append(os.path.join(folder, f))
    out = []
    for path in sorted(found):
        city = os.path.relpath(os.path.dirname(path), top)
        out.append(("" if city == "." else city, os.path.basename(path)[:-len(ID_SUFFIX)], path))
    return out


def read_id_map(path):
    """the map as uint16 [H, W]; Pillow modes I;16 and I (when every value fits 16 bits) — ValueError naming the file otherwise"""
    from PIL import Image

    with Image.open(path) as im:
        if im.mode not in ("I;16", "I;16L", "I;16B", "I"):       # (an 8-bit image holds no instance id: a labelIds map?)
            raise ValueError("%s: an id map is a 16- or 32-bit single-channel image, not mode %s" % (path, im.mode))
        return _as_uint16(np.array(im), path)


def image_name(stem, variant="plain", beta=0.02):
    if variant not in VARIANTS:
        raise ValueError("variant must be one of %s, got %r" % (VARIANTS, variant))
    if variant != "foggy":
        return stem + "_leftImg8bit.png"                  # rainy renderings keep the plain name
    match = [b for b in BETAS if abs(float(beta) - b) < 1e-12]
    if not match:
        raise ValueError("beta must be one of %s, got %r" % (BETAS, beta))
    return "%s_leftImg8bit_foggy_beta_%s.png" % (stem, repr(match[0]))


def _is_flat(image_dir):
    """no per-city folders: the images lie directly in image_dir (what the reference's json assumes)"""
    return any(f.lower().endswith(".png") for f in os.listdir(image_dir) if os.path.isfile(os.path.join(image_dir, f)))


def annotations_from_tables(entries, tables, sizes, variant="plain", beta=0.02, car_only=False, drop_fragmented=True, flat=True):
    """entries: `list_id_maps`; tables[i] / sizes[i]: the instance table and (H, W) of map i -> the COCO-format dict"""
    names = ("car",) if car_only else CATEGORIES
    category_of = {LABEL_IDS[name]: i + 1 for i, name in enumerate(names)}
    images, annotations = [], []
    for img_id, ((city, stem, _), table, (H, W)) in enumerate(zip(entries, tables, sizes)):
        base = image_name(stem, variant, beta)
        images.append({"id": img_id, "width": int(W), "height": int(H),
                       "file_name": base if flat or not city else city + "/" + base,
                       "seg_file_name": stem + ID_SUFFIX})
        for inst, x0, y0, x1, y1, count, fragmented in np.asarray(table).tolist():
            category = category_of.get(inst // 1000)
            if category is None or (fragmented and drop_fragmented):
                continue
            annotations.append({"id": len(annotations), "image_id": img_id, "category_id": category, "iscrowd": 0,
                                "area": count, "bbox": [x0, y0, x1 - x0 + 1, y1 - y0 + 1]})
    return {"images": images, "categories": [{"id": i + 1, "name": name} for i, name in enumerate(names)],
            "annotations": annotations}


def build_annotations(gt_dir, split, variant="plain", beta=0.02, car_only=False, drop_fragmented=True, image_dir=None,
                      device=None, timings=None):
    """gt_dir holds <split>/<city>/*_gtFine_instanceIds.png -> {"images", "categories", "annotations"} in COCO format (bbox,
    area, iscrowd, category_id, id, image_id; no segmentation).  image_dir: where the split's images lie, only looked at to
    decide between `file_name` = basename (flat directory) and <city>/<basename>; None: basenames.  device: None = the HIP
    device when one is present and the library is built, else the host; "cpu" or a HIP device to choose.  timings: a dict that
    receives the seconds spent decoding the maps (`decode_s`) and computing their tables (`tables_s`: staging, upload, launches
    and the wait on the device path) — tools/probes/cityscapes_boxes_time.py reads it."""
    image_name("x", variant, beta)                       # validate before any file is read
    entries = list_id_maps(gt_dir, split)
    use_device = device_available() if device is None else str(device) != "cpu"
    buffers = DeviceTables("cuda" if device is None else device) if use_device and entries else None
    tables, sizes = [], []
    phases = [0.0, 0.0] if timings is not None else None
    for at in range(0, len(entries), BATCH):
        t0 = time.perf_counter()
        maps = [read_id_map(path) for _, _, path in entries[at:at + BATCH]]
        t1 = time.perf_counter()
        sizes.extend(m.shape for m in maps)
        tables.extend(buffers.tables(maps) if use_device else [instance_table_host(m) for m in maps])
        if phases is not None:
            phases[0] += t1 - t0
            phases[1] += time.perf_counter() - t1
    if timings is not None:
        timings.update(decode_s=phases[0], tables_s=phases[1])
    flat = True if image_dir is None or not os.path.isdir(image_dir) else _is_flat(image_dir)
    return annotations_from_tables(entries, tables, sizes, variant, beta, car_only, drop_fragmented, flat)


# ----------------------------------------------------------------------------------------------------- dataset
def parse_options(text):
    """`SPLIT[,foggy[=BETA]|rain][,caronly]` (what follows `cityscapes:ROOT,` on the tools' command lines)
    -> dict(split=, variant=, beta=, car_only=)"""
    parts = [p.strip() for p in text.split(",")]
    if not parts[0]:
        raise ValueError("cityscapes:ROOT,SPLIT — the split is missing")
    out = dict(split=parts[0], variant="plain", beta=0.02, car_only=False)
    for p in parts[1:]:
        if p == "caronly":
            out["car_only"] = True
        elif p == "rain" or p == "foggy" or p.startswith("foggy="):
            if out["variant"] != "plain":
                raise ValueError("cityscapes spec: more than one of foggy / rain in %r" % text)
            out["variant"] = p.split("=")[0]
            if "=" in p:
                out["beta"] = float(p.split("=", 1)[1])
        else:
            raise ValueError("cityscapes spec: unknown option %r (foggy[=BETA], rain, caronly)" % p)
    image_name("x", out["variant"], out["beta"])
    return out


class CityscapesDataset(COCODataset):
    """Cityscapes in the layout of its archives: root/gtFine/<split>/<city>/*_gtFine_instanceIds.png and
    root/leftImg8bit[_foggy|_rain]/<split>/[<city>/]*.png.  The annotations are built when the dataset is (`build_annotations`);
    everything else — samples, domain flag, decode_to_tensor, get_groundtruth, id maps, category tables — is COCODataset's."""

    def __init__(self, root, split, variant="plain", beta=0.02, car_only=False, remove_images_without_annotations=False,
                 transforms=None, is_source=True, decode_to_tensor=False, drop_fragmented=True, device=None):
        if variant not in VARIANTS:
            raise ValueError("variant must be one of %s, got %r" % (VARIANTS, variant))
        image_dir = os.path.join(root, IMAGE_DIRS[variant], split)
        data = build_annotations(os.path.join(root, "gtFine"), split, variant, beta, car_only, drop_fragmented, image_dir, device)
        super(CityscapesDataset, self).__init__(data, image_dir, remove_images_without_annotations, transforms, is_source,
                                                decode_to_tensor)
        self.split, self.variant, self.beta, self.car_only = split, variant, beta, car_only


def json_name(dataset, split):
    """the reference converters' file names"""
    pattern = {"cityscapes_instance_only": "instancesonly_filtered_gtFine_%s.json",
               "foggy_cityscapes": "foggy_instancesonly_filtered_gtFine_%s.json",
               "cityscapes_car_only": "caronly_filtered_gtFine_%s.json"}[dataset]
    return pattern % split


def write_json(data, path):
    with open(path, "w") as f:
        f.write(json.dumps(data))


def write_annotation_file(root, options, path, device=None):
    """the set `cityscapes:ROOT,<options>` names, as an (annotation file, image root) pair: its annotations are written to
    `path` -> (path, ROOT/leftImg8bit[_foggy|_rain]/<split>) — for tools that take annotation files (tools/test_net_da.py)"""
    opts = parse_options(options)
    image_dir = os.path.join(root, IMAGE_DIRS[opts["variant"]], opts["split"])
    write_json(build_annotations(os.path.join(root, "gtFine"), opts["split"], opts["variant"], opts["beta"], opts["car_only"],
                                 True, image_dir, device), path)
    return path, image_dir
