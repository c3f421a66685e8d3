"""Detections drawn onto images: the draw list, its placement rules, a host renderer and the device renderer
(reference: demo/predictor.py:235-283,358-383 `select_top_predictions`, `compute_colors_for_labels`, `overlay_boxes`,
`overlay_class_names`, which draw with cv2).

This module owns every placement decision.  A *draw record* (`DrawRecord`) is one box: inclusive integer corners that may lie
partly or wholly outside the image, a colour, an outline thickness `w` (1 .. 8), a fill opacity `a` (0 .. 256, 0: no tint),
a label of printable ASCII (at most 64 characters) and the origin (tx, ty) of the label's first 6 x 11 glyph cell.

Per pixel (x, y) with value v, the records taken in list order, c a record's colour — the same for both renderers:

  pass A, every record:
    tint     a > 0 and x0 <= x <= x1 and y0 <= y <= y1:   v = (c * a + v * (256 - a) + 128) >> 8   per channel
    outline  inside the box and (x - x0 < w or x1 - x < w or y - y0 < w or y1 - y < w):   v = c
  pass B, after ALL of pass A, every record with a non-empty label:
    plate    tx - 1 <= x <= tx + 6 * len and ty - 1 <= y <= ty + 11:   v = c
    ink      bit ((x - tx) % 6, y - ty) of the glyph of character (x - tx) // 6 is set:   v = ink, where
             ink = white when (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16 < 128 (Pillow's L), else black

Pixels no record covers keep their bytes.  On every box at least 2 w wide and high the outline is what Pillow's
`ImageDraw.rectangle(outline=, width=w)` draws; a thinner box is filled and nothing outside it changes.

Deviations from the reference, both deliberate: records are painted by ASCENDING score, so the most confident box lies on top
(the reference paints it first); the text is this project's glyph cells (engine/_glyphs.py) on a plate in the box colour, not
cv2's Hershey strokes.

`render_host` is the numpy statement of the rule; `render_device` runs csrc/overlay.hip (`dadet_overlay_batch`) on uint8
[H][W][3] device tensors in place.  They give the same bytes (tests/test_overlay_gpu.py)."""
import collections
import ctypes

import numpy as np

from .. import _lib
from . import _glyphs

MAX_RECORDS = _lib.OVERLAY_MAX_RECORDS      # per image; the host renderer keeps the device's limits
MAX_LABEL = _lib.OVERLAY_MAX_LABEL
MAX_THICKNESS = 8
CELL_W, CELL_H = _glyphs.CELL_W, _glyphs.CELL_H
# corners further out than this are pulled in: no image reaches that far (H * W <= 2^28), so nothing visible moves, and
# every difference the rule takes fits 32 bits
_CORNER_LIMIT = 1 << 30

DrawRecord = collections.namedtuple("DrawRecord", ["x0", "y0", "x1", "y1", "color", "w", "a", "label", "tx", "ty"])


# ------------------------------------------------------------------------------------------------------------ the rules
def sanitize_label(text):
    """printable ASCII stays, any other character becomes `?`; more than MAX_LABEL characters is an error"""
    text = "".join(ch if 0x20 <= ord(ch) <= 0x7e else "?" for ch in str(text))
    if len(text) > MAX_LABEL:
        raise ValueError("label of %d characters (at most %d)" % (len(text), MAX_LABEL))
    return text


def place_label(x0, y0, w):
    """cell origin (tx, ty) of the label of a box with top-left corner (x0, y0) and outline w: the plate
    [tx - 1, ty - 1, tx + 6 * len, ty + 11] sits directly above the box, or — when its top row would lie above row 0 — inside
    the box under the outline.  Nothing is clamped on the right or at the bottom: the image clips the label there."""
    tx = max(x0, 0) + 1
    ty = y0 - (CELL_H + 1)
    if ty - 1 < 0:
        ty = max(y0, 0) + w + 1
    return tx, ty


def ink_for(color):
    r, g, b = (int(v) for v in color)
    return (255, 255, 255) if (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16 < 128 else (0, 0, 0)


def make_record(box, color, label="", thickness=2, fill_alpha=0):
    """box: four integers x0, y0, x1, y1 (inclusive corners) -> DrawRecord with its label placed"""
    x0, y0, x1, y1 = (max(-_CORNER_LIMIT, min(_CORNER_LIMIT, int(v))) for v in box)
    w, a = int(thickness), int(fill_alpha)
    if not 1 <= w <= MAX_THICKNESS:
        raise ValueError("outline thickness %d (1 .. %d)" % (w, MAX_THICKNESS))
    if not 0 <= a <= 256:
        raise ValueError("fill opacity %d (0 .. 256)" % a)
    color = tuple(int(v) for v in color)
    if len(color) != 3 or any(not 0 <= v <= 255 for v in color):
        raise ValueError("colour %r is not three bytes" % (color,))
    tx, ty = place_label(x0, y0, w)
    return DrawRecord(x0, y0, x1, y1, color, w, a, sanitize_label(label), tx, ty)


_PALETTE = (2 ** 25 - 1, 2 ** 15 - 1, 2 ** 21 - 1)


def compute_colors_for_labels(labels):
    """predictor.py:256-262: labels[:, None] * palette % 255, i.e. label k -> (k, 127 k, 31 k) mod 255.  The reference hands
    that triple to cv2 as B, G, R; the images here are RGB, so it is stored reversed: uint8 [N, 3] RGB, label 1 ->
    (31, 127, 1)."""
    labels = np.asarray(labels.cpu() if hasattr(labels, "cpu") else labels, dtype=np.int64).reshape(-1)
    bgr = labels[:, None] * np.asarray(_PALETTE, dtype=np.int64)[None, :] % 255
    return np.ascontiguousarray(bgr[:, ::-1]).astype(np.uint8)


def select_top_predictions(boxlist, threshold):
    """predictor.py:235-254: the predictions with `scores` > threshold, in descending order of score"""
    import torch

    scores = boxlist.get_field("scores")
    kept = boxlist[torch.nonzero(scores > threshold).squeeze(1)]
    _, order = kept.get_field("scores").sort(0, descending=True)
    return kept[order]


def build_draw_list(boxlist, categories=None, thickness=2, fill_alpha=0, show_scores=True, colors=None):
    """BoxList (xyxy or xywh; `labels`, optionally `scores`) -> list of DrawRecord.  Corners are `box.to(int64)`
    (predictor.py:279).  Label: "{name} {score:.2f}", the name alone without scores (ground truth) or with
    show_scores=False, the numeric label when `categories` has no name for it (categories: a sequence indexed by label, or
    a mapping).  colors: uint8 [N, 3] RGB to use instead of compute_colors_for_labels.  Records are ordered by ASCENDING
    score — the most confident box is painted last and lies on top; a BoxList without `scores` keeps its own order."""
    import torch

    boxlist = boxlist.convert("xyxy")
    n = len(boxlist)
    if n > MAX_RECORDS:
        raise ValueError("%d boxes on one image (at most %d)" % (n, MAX_RECORDS))
    boxes = boxlist.bbox.detach().cpu().to(torch.int64).tolist()
    labels = [int(v) for v in boxlist.get_field("labels").tolist()] if boxlist.has_field("labels") else [0] * n
    scores = [float(v) for v in boxlist.get_field("scores").tolist()] if boxlist.has_field("scores") else None
    if colors is None:
        colors = compute_colors_for_labels(labels)
    colors = np.asarray(colors).reshape(n, 3)

    def name_of(label):
        if categories is not None:
            try:
                return str(categories[label])
            except (IndexError, KeyError):
                pass
        return str(label)

    order = list(range(n))
    if scores is not None:
        order.sort(key=lambda i: scores[i])            # stable: equal scores keep the list's order
    records = []
    for i in order:
        text = name_of(labels[i])
        if scores is not None and show_scores:
            text = "%s %.2f" % (text, scores[i])
        records.append(make_record(boxes[i], colors[i], text, thickness, fill_alpha))
    return records


def boxes_only(records):
    """the records without their labels: pass A alone (the reference's overlay_boxes)"""
    return [r._replace(label="") for r in records]


def labels_only(records):
    """the records with an empty box, labels where the real box put them: pass B alone (the reference's
    overlay_class_names).  Pass B comes after all of pass A, so drawing boxes_only and then labels_only gives the bytes of
    drawing the records at once."""
    return [r._replace(x0=0, y0=0, x1=-1, y1=-1) for r in records]


def _check_list(records):
    if len(records) > MAX_RECORDS:
        raise ValueError("%d records on one image (at most %d)" % (len(records), MAX_RECORDS))
    for r in records:
        if len(r.label) > MAX_LABEL:
            raise ValueError("label of %d characters (at most %d)" % (len(r.label), MAX_LABEL))


# --------------------------------------------------------------------------------------------------------------- the host
def _clip(xa, ya, xb, yb, W, H):
    """inclusive rectangle cut by the image -> slices, or None when nothing is left"""
    xa, ya, xb, yb = max(xa, 0), max(ya, 0), min(xb, W - 1), min(yb, H - 1)
    if xa > xb or ya > yb:
        return None
    return slice(ya, yb + 1), slice(xa, xb + 1)


def render_host(image_u8_hwc, records, inplace=False):
    """uint8 [H, W, 3] numpy array + draw list -> the drawn image: the array itself with inplace=True, else a copy"""
    img = image_u8_hwc if inplace else np.array(image_u8_hwc, dtype=np.uint8, order="C")
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    _check_list(records)
    H, W = img.shape[:2]
    for r in records:                                           # pass A
        if r.x1 < r.x0 or r.y1 < r.y0:
            continue
        c = np.asarray(r.color, dtype=np.uint8)
        if r.a > 0:
            s = _clip(r.x0, r.y0, r.x1, r.y1, W, H)
            if s is not None:
                v = img[s].astype(np.int32)
                img[s] = ((c.astype(np.int32) * r.a + v * (256 - r.a) + 128) >> 8).astype(np.uint8)
        w = r.w
        for band in ((r.x0, r.y0, r.x1, min(r.y0 + w - 1, r.y1)), (r.x0, max(r.y1 - w + 1, r.y0), r.x1, r.y1),
                     (r.x0, r.y0, min(r.x0 + w - 1, r.x1), r.y1), (max(r.x1 - w + 1, r.x0), r.y0, r.x1, r.y1)):
            s = _clip(*band, W, H)
            if s is not None:
                img[s] = c
    for r in records:                                           # pass B
        n = len(r.label)
        if n == 0:
            continue
        s = _clip(r.tx - 1, r.ty - 1, r.tx + CELL_W * n, r.ty + CELL_H, W, H)
        if s is None:
            continue
        img[s] = np.asarray(r.color, dtype=np.uint8)
        ink = np.asarray(ink_for(r.color), dtype=np.uint8)
        for k, ch in enumerate(r.label):
            cx = r.tx + CELL_W * k
            s = _clip(cx, r.ty, cx + CELL_W - 1, r.ty + CELL_H - 1, W, H)
            if s is None:
                continue
            rows = _glyphs.GLYPHS[ord(ch) - _glyphs.FIRST]
            cell = (rows[:, None] >> (CELL_W - 1 - np.arange(CELL_W))[None, :]) & 1
            mask = cell[s[0].start - r.ty:s[0].stop - r.ty, s[1].start - cx:s[1].stop - cx].astype(bool)
            img[s][mask] = ink
    return img


# ------------------------------------------------------------------------------------------------------------- the device
RECORD_INTS = 12        # DADET_OVERLAY_RECORD_INTS: x0 y0 x1 y1 rgb w a tx ty text_offset text_length 0
DEVICE_CHUNK = 256      # DADET_OVERLAY_CHUNK: records culled per round of the kernel (tests need more than one round)


def pack_records(record_lists):
    """draw lists, one per image -> (int32 [total, RECORD_INTS], text bytes, [(first, count) per image]); the colour is
    r | g << 8 | b << 16, a label's bytes lie at text[text_offset : text_offset + text_length]"""
    rows, text, ranges = [], bytearray(), []
    for records in record_lists:
        _check_list(records)
        ranges.append((len(rows), len(records)))
        for r in records:
            rows.append((r.x0, r.y0, r.x1, r.y1, r.color[0] | r.color[1] << 8 | r.color[2] << 16, r.w, r.a, r.tx, r.ty,
                         len(text), len(r.label), 0))
            text += sanitize_label(r.label).encode("ascii")
    packed = np.asarray(rows, dtype=np.int32).reshape(len(rows), RECORD_INTS)
    return packed, bytes(text), ranges


def render_device(images, record_lists):
    """images: uint8 [H, W, 3] contiguous device tensors, drawn IN PLACE; record_lists: one draw list per image.  One upload
    (packed records, glyph table, text bytes — one buffer) for the whole call and one dadet_overlay_batch launch per
    _lib.OVERLAY_BATCH_MAX images on the current stream; an image without records is not touched.  Returns `images`."""
    import torch

    images = list(images)
    assert len(images) == len(record_lists)
    if not images:
        return images
    dev = images[0].device
    for img in images:
        if not img.is_cuda:
            raise _lib.DadetError("render_device: the images must live on the HIP device")
        assert img.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == 3 and img.device == dev
        if not img.is_contiguous():
            raise ValueError("render_device draws in place: the image tensors must be contiguous")
    packed, text, ranges = pack_records(record_lists)
    if packed.shape[0] == 0:
        return images
    glyph_at = packed.nbytes
    text_at = glyph_at + (_glyphs.GLYPHS.size + 3) // 4 * 4
    host = np.zeros(text_at + max(len(text), 1), dtype=np.uint8)
    host[:glyph_at] = packed.reshape(-1).view(np.uint8)
    host[glyph_at:glyph_at + _glyphs.GLYPHS.size] = _glyphs.GLYPHS.reshape(-1)
    host[text_at:text_at + len(text)] = np.frombuffer(text, dtype=np.uint8)
    buf = torch.from_numpy(host).to(dev)
    cur = torch.cuda.current_stream(dev)
    base = buf.data_ptr()
    for first in range(0, len(images), _lib.OVERLAY_BATCH_MAX):
        chunk = range(first, min(first + _lib.OVERLAY_BATCH_MAX, len(images)))
        if not any(ranges[i][1] for i in chunk):
            continue
        items = (_lib.OverlayItem * len(chunk))()
        for it, i in zip(items, chunk):
            it.image, it.H, it.W = images[i].data_ptr(), int(images[i].shape[0]), int(images[i].shape[1])
            it.first, it.count = ranges[i]
        _lib.call("dadet_overlay_batch", items, len(chunk), ctypes.c_void_p(base), ctypes.c_void_p(base + text_at),
                  ctypes.c_void_p(base + glyph_at), ctypes.c_void_p(cur.cuda_stream))
    for t in images + [buf]:
        t.record_stream(cur)
    return images
