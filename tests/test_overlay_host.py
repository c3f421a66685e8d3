"""Drawing detections, host side: the rules of engine/overlay.py against Pillow's ImageDraw where they are
meant to agree, against hand-computed bytes, and against the rule read pixel by pixel (_overlay_cases.reference_render);
the glyph table against Pillow's bitmap font; the ABI of dadet_overlay_batch; tools/draw_detections.py --host."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image, ImageDraw, ImageFont

import _overlay_cases as C
from da_detect_amd.engine import _glyphs, overlay
from da_detect_amd.engine.overlay import DrawRecord, make_record, render_host
from da_detect_amd.structures.bounding_box import BoxList

ROOT = C.ROOT


def _pil(image):
    return Image.fromarray(np.array(image))


# ------------------------------------------------------------------------------------------------------------- pass A
def test_outline_equals_pillow_rectangle():
    """3000 seeded boxes, clipped and outside ones included, each at least 2 w wide and high: exact equality"""
    rng = np.random.default_rng(1)
    done = 0
    while done < 3000:
        H, W = (int(v) for v in rng.integers(1, 41, 2))
        w = int(rng.integers(1, 6))
        x0, x1 = np.sort(rng.integers(-10, 50, 2))
        y0, y1 = np.sort(rng.integers(-10, 50, 2))
        if x1 - x0 + 1 < 2 * w or y1 - y0 + 1 < 2 * w:
            continue
        done += 1
        bg = C.background(rng, H, W)
        color = tuple(int(v) for v in rng.integers(0, 256, 3))
        want = _pil(bg)
        ImageDraw.Draw(want).rectangle([int(x0), int(y0), int(x1), int(y1)], outline=color, width=w)
        got = render_host(bg, [make_record((x0, y0, x1, y1), color, "", thickness=w)])
        assert np.array_equal(got, np.array(want)), (H, W, x0, y0, x1, y1, w)


def test_thin_box_is_filled_and_stays_inside():
    rng = np.random.default_rng(2)
    for _ in range(300):
        H, W = 30, 30
        w = int(rng.integers(2, 6))
        x0, y0 = (int(v) for v in rng.integers(-5, 25, 2))
        x1, y1 = x0 + int(rng.integers(0, 2 * w - 1)), y0 + int(rng.integers(0, 12))      # narrower than 2 w
        bg = C.background(rng, H, W)
        got = render_host(bg, [make_record((x0, y0, x1, y1), (9, 8, 7), "", thickness=w)])
        inside = np.zeros((H, W), bool)
        inside[max(y0, 0):max(y1 + 1, 0), max(x0, 0):max(x1 + 1, 0)] = True
        assert np.array_equal(got[~inside], bg[~inside])
        assert (got[inside] == (9, 8, 7)).all()            # every pixel of the box is within w of one of its vertical edges


def test_plate_equals_pillow_filled_rectangle():
    """a label of spaces has no ink: its plate alone, against ImageDraw.rectangle(fill=)"""
    rng = np.random.default_rng(3)
    for _ in range(1000):
        H, W = (int(v) for v in rng.integers(1, 41, 2))
        n = int(rng.integers(1, 7))
        tx, ty = (int(v) for v in rng.integers(-45, 50, 2))
        color = tuple(int(v) for v in rng.integers(0, 256, 3))
        bg = C.background(rng, H, W)
        want = _pil(bg)
        ImageDraw.Draw(want).rectangle([tx - 1, ty - 1, tx + 6 * n, ty + 11], fill=color)
        got = render_host(bg, [DrawRecord(0, 0, -1, -1, color, 2, 0, " " * n, tx, ty)])
        assert np.array_equal(got, np.array(want)), (H, W, tx, ty, n)


def test_tint_closed_form():
    bg = np.zeros((12, 12, 3), np.uint8)
    bg[:] = (10, 200, 77)
    got = render_host(bg, [make_record((1, 1, 10, 10), (255, 0, 128), "", thickness=2, fill_alpha=64)])
    # (255 * 64 + 10 * 192 + 128) >> 8 = 18368 >> 8 = 71;  (200 * 192 + 128) >> 8 = 150;  (128 * 64 + 77 * 192 + 128) >> 8 = 90
    assert tuple(got[5, 5]) == (71, 150, 90)
    assert tuple(got[1, 5]) == tuple(got[2, 5]) == tuple(got[5, 10]) == (255, 0, 128)        # the outline, 2 wide
    assert tuple(got[0, 0]) == tuple(got[11, 5]) == (10, 200, 77)                            # outside
    solid = render_host(bg, [make_record((1, 1, 10, 10), (255, 0, 128), "", thickness=1, fill_alpha=256)])
    assert (solid[1:11, 1:11] == (255, 0, 128)).all()                                       # a = 256 gives exactly c
    clear = render_host(bg, [make_record((1, 1, 10, 10), (255, 0, 128), "", thickness=1, fill_alpha=0)])
    assert (clear[2:10, 2:10] == (10, 200, 77)).all()                                       # a = 0 changes nothing
    for bad in (-1, 257):
        with pytest.raises(ValueError):
            make_record((1, 1, 10, 10), (1, 2, 3), fill_alpha=bad)
    for bad in (0, 9):
        with pytest.raises(ValueError):
            make_record((1, 1, 10, 10), (1, 2, 3), thickness=bad)


def test_paint_order():
    bg = np.full((20, 20, 3), 100, np.uint8)
    red = make_record((0, 0, 15, 15), (255, 0, 0), "", thickness=1, fill_alpha=128)
    blue = make_record((4, 4, 19, 19), (0, 0, 255), "", thickness=1, fill_alpha=128)
    # red first: (255 * 128 + 100 * 128 + 128) >> 8 = 178, (100 * 128 + 128) >> 8 = 50; then blue over (178, 50, 50):
    # (178 * 128 + 128) >> 8 = 89, (50 * 128 + 128) >> 8 = 25, (255 * 128 + 50 * 128 + 128) >> 8 = 153
    assert tuple(render_host(bg, [red, blue])[10, 10]) == (89, 25, 153)
    assert tuple(render_host(bg, [blue, red])[10, 10]) == (153, 25, 89)
    # pass B lies over pass A of a LATER record: the first record's plate covers the second one's outline and tint
    first = make_record((2, 14, 18, 18), (0, 255, 0), "  ", thickness=1)          # plate above its box: rows 1 .. 13
    assert (first.tx, first.ty) == (3, 2)
    later = make_record((0, 0, 19, 19), (255, 0, 255), "", thickness=3, fill_alpha=256)
    got = render_host(bg, [first, later])
    assert (got[1:14, 2:16] == (0, 255, 0)).all()
    assert tuple(got[0, 5]) == tuple(got[5, 17]) == (255, 0, 255)


# ------------------------------------------------------------------------------------------------------------- labels
def test_glyph_table_equals_pillow_bitmap_font():
    font = ImageFont.load_default_imagefont()
    assert _glyphs.GLYPHS.shape == (95, 11) and _glyphs.GLYPHS.dtype == np.uint8 and int(_glyphs.GLYPHS.max()) < 64
    for code in range(0x20, 0x7f):
        cell = Image.new("1", (6, 11), 0)
        ImageDraw.Draw(cell).text((0, 0), chr(code), fill=1, font=font)
        want = np.array(cell, dtype=np.uint8)
        rows = _glyphs.GLYPHS[code - 0x20]
        got = (rows[:, None] >> (5 - np.arange(6))[None, :]) & 1
        assert np.array_equal(got, want), chr(code)


def test_label_placement():
    assert overlay.place_label(20, 30, 2) == (21, 18)                  # above the box: plate rows 17 .. 29
    assert overlay.place_label(20, 13, 2) == (21, 1)                   # plate top exactly at row 0
    assert overlay.place_label(20, 12, 2) == (21, 15)                  # one higher would leave the image: inside, under the outline
    assert overlay.place_label(20, -7, 3) == (21, 4)
    assert overlay.place_label(-9, 40, 2) == (1, 28)                   # x0 < 0
    r = make_record((20, 30, 60, 50), (1, 2, 3), "ab")
    assert (r.tx, r.ty, r.label) == (21, 18, "ab")
    assert make_record((0, 0, 5, 5), (1, 2, 3), "café\t\x7f").label == "caf???"      # non-ASCII, control, DEL
    make_record((0, 0, 5, 5), (1, 2, 3), "x" * 64)
    with pytest.raises(ValueError):
        make_record((0, 0, 5, 5), (1, 2, 3), "x" * 65)
    with pytest.raises(ValueError):
        render_host(np.zeros((4, 4, 3), np.uint8), [make_record((0, 0, 1, 1), (1, 2, 3))] * 1025)
    with pytest.raises(ValueError):
        overlay.pack_records([[make_record((0, 0, 1, 1), (1, 2, 3))] * 1025])
    render_host(np.zeros((4, 4, 3), np.uint8), [make_record((0, 0, 1, 1), (1, 2, 3))] * 1024)


def test_labels_clipped_by_the_image_and_ink_colour():
    rng = np.random.default_rng(4)
    bg = C.background(rng, 40, 60)
    records = [make_record((40, 20, 58, 30), (250, 250, 10), "right edge"),       # runs off the right edge
               make_record((5, 3, 30, 12), (10, 10, 120), "top"),                 # inside the box
               make_record((-9, 25, 20, 45), (200, 30, 30), "x0<0"),
               make_record((30, 38, 50, 70), (0, 0, 0), "low")]                   # box below; plate rows 25 .. 37
    low = DrawRecord(10, 50, 20, 60, (255, 255, 255), 2, 0, "bottom", 11, 33)     # partly below the bottom edge
    got = render_host(bg, records + [low])
    assert np.array_equal(got, C.reference_render(bg, records + [low]))
    assert tuple(got[39, 10]) == (255, 255, 255) and overlay.ink_for((255, 255, 255)) == (0, 0, 0)
    assert overlay.ink_for((10, 10, 120)) == (255, 255, 255) and overlay.ink_for((250, 250, 10)) == (0, 0, 0)
    # L = (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16: (128, 128, 128) -> 128, black ink; (127, 127, 127) -> white
    assert overlay.ink_for((128, 128, 128)) == (0, 0, 0) and overlay.ink_for((127, 127, 127)) == (255, 255, 255)
    assert (got[6:17, 6:24] == 255).all(axis=2).any()                             # white ink on the dark plate of "top"


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_render_host_equals_the_rule_read_per_pixel(seed):
    rng = np.random.default_rng(100 + seed)
    H, W = (int(v) for v in rng.integers(8, 36, 2))
    bg = C.background(rng, H, W)
    records = C.random_records(rng, 12, H, W)
    assert np.array_equal(render_host(bg, records), C.reference_render(bg, records))
    again = bg.copy()
    assert render_host(again, records, inplace=True) is again and not np.array_equal(again, bg)


def test_boxes_then_labels_is_the_whole():
    rng = np.random.default_rng(5)
    bg = C.background(rng, 30, 50)
    records = C.random_records(rng, 8, 30, 50)
    two_steps = render_host(render_host(bg, overlay.boxes_only(records)), overlay.labels_only(records))
    assert np.array_equal(two_steps, render_host(bg, records))


# ----------------------------------------------------------------------------------------------- colours and draw lists
def test_compute_colors_for_labels():
    colors = overlay.compute_colors_for_labels(torch.arange(0, 301))
    assert colors.dtype == np.uint8 and colors.shape == (301, 3)
    assert tuple(colors[1]) == (31, 127, 1) and tuple(colors[255]) == (0, 0, 0)
    palette = torch.tensor([2 ** 25 - 1, 2 ** 15 - 1, 2 ** 21 - 1])
    reference = ((torch.arange(0, 301)[:, None] * palette) % 255).numpy().astype("uint8")       # handed to cv2 as B, G, R
    assert np.array_equal(colors, reference[:, ::-1])


def _boxlist():
    b = BoxList(torch.tensor([[1.9, 2.2, 30.7, 40.1], [-3.5, 5.0, 10.0, 20.0], [4.0, 4.0, 9.0, 9.0], [0.0, 0.0, 5.0, 5.0]]),
                (64, 48))
    b.add_field("labels", torch.tensor([1, 2, 3, 1]))
    b.add_field("scores", torch.tensor([0.9, 0.95, 0.3, 0.7]))
    return b


def test_select_top_predictions_and_draw_list_order():
    top = overlay.select_top_predictions(_boxlist(), 0.7)                # strictly above: 0.7 itself goes
    assert top.get_field("scores").tolist() == pytest.approx([0.95, 0.9])
    assert top.get_field("labels").tolist() == [2, 1]
    records = overlay.build_draw_list(top, ["bg", "person", "car"])
    assert [r.label for r in records] == ["person 0.90", "car 0.95"]     # ascending: the most confident painted last
    assert (records[0].x0, records[0].y0, records[0].x1, records[0].y1) == (1, 2, 30, 40)      # box.to(int64) truncates
    assert (records[1].x0, records[1].tx) == (-3, 1)
    assert records[0].color == (31, 127, 1) and records[0].w == 2 and records[0].a == 0
    assert [r.label for r in overlay.build_draw_list(top, ["bg", "person", "car"], show_scores=False)] == ["person", "car"]
    assert [r.label for r in overlay.build_draw_list(top)] == ["1 0.90", "2 0.95"]              # no names: the label
    assert [r.label for r in overlay.build_draw_list(top, {2: "car"})] == ["1 0.90", "car 0.95"]
    gt = _boxlist().copy_with_fields(["labels"])
    records = overlay.build_draw_list(gt, ["bg", "person", "car", "bus"], thickness=3, fill_alpha=40,
                                      colors=np.arange(12).reshape(4, 3))
    assert [r.label for r in records] == ["person", "car", "bus", "person"]                     # its own order
    assert records[2].color == (6, 7, 8) and records[2].w == 3 and records[2].a == 40
    assert overlay.build_draw_list(overlay.select_top_predictions(_boxlist(), 0.99)) == []


def test_pack_records_layout():
    a = make_record((1, 2, 3, 4), (10, 20, 30), "ab", thickness=3, fill_alpha=7)
    b = make_record((-5, 6, 7, 80), (1, 2, 3), "", thickness=1)
    c = make_record((0, 0, 9, 9), (255, 255, 255), "xyz")
    packed, text, ranges = overlay.pack_records([[a, b], [], [c]])
    assert packed.dtype == np.int32 and packed.shape == (3, overlay.RECORD_INTS) and ranges == [(0, 2), (2, 0), (2, 1)]
    assert text == b"abxyz"
    assert packed[0].tolist() == [1, 2, 3, 4, 10 | 20 << 8 | 30 << 16, 3, 7, a.tx, a.ty, 0, 2, 0]
    assert packed[1].tolist()[9:11] == [2, 0] and packed[2].tolist()[9:11] == [2, 3]


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_overlay_abi():
    from da_detect_amd import _lib

    header = open(os.path.join(ROOT, "include", "dadet.h")).read()
    name = "dadet_overlay_batch"
    proto = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
    assert proto, "include/dadet.h does not declare %s" % name
    assert len(proto.group(1).split(",")) == len(_lib._SIGNATURES[name]) == 6
    assert name in _lib.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert "overlay.hip" in open(os.path.join(ROOT, "da_detect_amd", "csrc", "Makefile")).read()
    for constant, value, mirror in (("DADET_OVERLAY_BATCH_MAX", 8, _lib.OVERLAY_BATCH_MAX),
                                    ("DADET_OVERLAY_MAX_RECORDS", 1024, _lib.OVERLAY_MAX_RECORDS),
                                    ("DADET_OVERLAY_MAX_LABEL", 64, _lib.OVERLAY_MAX_LABEL),
                                    ("DADET_OVERLAY_RECORD_INTS", overlay.RECORD_INTS, overlay.RECORD_INTS),
                                    ("DADET_OVERLAY_CHUNK", overlay.DEVICE_CHUNK, overlay.DEVICE_CHUNK)):
        assert int(re.search(r"#define %s (\d+)" % constant, header).group(1)) == value == mirror
    assert (overlay.MAX_RECORDS, overlay.MAX_LABEL) == (_lib.OVERLAY_MAX_RECORDS, _lib.OVERLAY_MAX_LABEL)
    assert ctypes.sizeof(_lib.OverlayItem) == 24


# --------------------------------------------------------------------------------------------------------------- tool
@pytest.fixture(scope="module")
def coco_set(tmp_path_factory):
    return C.write_coco_set(tmp_path_factory.mktemp("overlay_set"))


def test_tool_host_panels(coco_set, tmp_path):
    tool = C.load_tool()
    out = str(tmp_path / "figs")
    written = tool.main(["--dataset", coco_set["spec"], "--predictions", coco_set["a"], "--out", out, "--gt", "--compare",
                         coco_set["b"], "--host"])
    assert [os.path.basename(p) for p in written] == ["frame_%d.png" % i for i in range(4)]
    assert sorted(os.listdir(out)) == ["frame_%d.png" % i for i in range(4)]
    drawn = 0
    for i, (H, W) in enumerate(C.SET_SIZES):
        got = np.array(Image.open(os.path.join(out, "frame_%d.png" % i)))
        assert got.shape == (3 * H, W, 3)
        want = C.expected_panels(coco_set, i, True, [coco_set["a"], coco_set["b"]])
        assert np.array_equal(got, want)
        original = np.array(Image.open(os.path.join(coco_set["img"], "frame_%d.png" % i)).convert("RGB"))
        drawn += sum(not np.array_equal(got[k * H:(k + 1) * H], original) for k in range(3))
    assert drawn >= 8                                  # the panels are not the bare images


def test_tool_selection_and_style(coco_set, tmp_path):
    tool = C.load_tool()
    out = str(tmp_path / "some")
    written = tool.main(["--dataset", coco_set["spec"], "--predictions", coco_set["a"], "--out", out, "--host", "--ids", "103",
                         "101", "--thickness", "3", "--fill-alpha", "64", "--no-scores", "--threshold", "0.6"])
    assert [os.path.basename(p) for p in written] == ["frame_1.png", "frame_3.png"] == sorted(os.listdir(out))
    for i in (1, 3):
        want = C.expected_panels(coco_set, i, False, [coco_set["a"]], threshold=0.6, thickness=3, fill_alpha=64,
                                 show_scores=False)
        assert np.array_equal(np.array(Image.open(os.path.join(out, "frame_%d.png" % i))), want)
    out = str(tmp_path / "few")
    written = tool.main(["--dataset", coco_set["spec"], "--predictions", coco_set["a"], "--out", out, "--host", "--limit", "2"])
    assert sorted(os.listdir(out)) == ["frame_0.png", "frame_1.png"]
    with pytest.raises(SystemExit):
        tool.main(["--dataset", coco_set["spec"], "--predictions", coco_set["a"], "--out", out, "--host", "--ids", "999"])
    with pytest.raises(SystemExit):
        tool.main(["--dataset", coco_set["spec"], "--out", out, "--host"])
