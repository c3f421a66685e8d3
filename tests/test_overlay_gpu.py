"""Drawing detections on the GPU: csrc/overlay.hip (dadet_overlay_batch — a workgroup per 16 x 64 pixel tile culls the
image's records DEVICE_CHUNK at a time into an ordered LDS list and applies pass A, then pass B, in registers) against
engine/overlay.py render_host, byte for byte, on random backgrounds so that untouched pixels are checked too; the tool and
COCODemo on top of it."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _overlay_cases as C
from da_detect_amd.engine import _glyphs, overlay
from da_detect_amd.engine.overlay import DrawRecord, make_record, render_host

pytestmark = pytest.mark.gpu


def _device_render(pixels, lists, device):
    """numpy images -> numpy results of ONE render_device call over all of them (launches of 8 inside)"""
    on_device = [torch.from_numpy(np.ascontiguousarray(p)).to(device) for p in pixels]
    out = overlay.render_device(on_device, lists)
    torch.cuda.synchronize()
    assert all(o is t for o, t in zip(out, on_device))                    # in place
    return [t.cpu().numpy() for t in on_device]


def _check(pixels, lists, device):
    got = _device_render(pixels, lists, device)
    for k, (p, records, g) in enumerate(zip(pixels, lists, got)):
        want = render_host(p, records)
        assert np.array_equal(g, want), "image %d (%d x %d): %d bytes differ" % (k, p.shape[0], p.shape[1], int((g != want).sum()))
    return got


WIDTHS = (1, 5, 61, 64, 65, 67, 130)


@pytest.mark.parametrize("H", [1, 15, 16, 17, 33])
def test_sizes_across_tile_and_alignment_edges(device, H):
    """one box spanning the image — plain, tinted, and tinted with a label — at every width: W * 3 is mostly no multiple of
    4, so rows start at every byte alignment; 61 .. 67 and 130 cross the 64-column tile, 15 .. 17 and 33 the 16-row one"""
    rng = np.random.default_rng(H)
    pixels, lists = [], []
    for W in WIDTHS:
        for style in (dict(), dict(fill_alpha=100), dict(fill_alpha=77, label="Wq%d" % W)):
            pixels.append(C.background(rng, H, W))
            lists.append([make_record((0, 0, W - 1, H - 1), (200, 40, 90), style.get("label", ""), thickness=1 + W % 3,
                                      fill_alpha=style.get("fill_alpha", 0))])
    _check(pixels, lists, device)


def test_image_memory_at_every_byte_offset(device):
    """images that start 0 .. 3 bytes into an allocation: the word path and the byte path of the loads and stores"""
    rng = np.random.default_rng(9)
    H, W = 19, 68                                                          # W * 3 = 204: a multiple of 4, rows keep the offset
    bg = C.background(rng, H, W)
    records = C.random_records(rng, 10, H, W)
    want = render_host(bg, records)
    for offset in range(4):
        buf = torch.zeros(H * W * 3 + 8, dtype=torch.uint8, device=device)
        view = buf[offset:offset + H * W * 3].view(H, W, 3)
        view.copy_(torch.from_numpy(bg))
        assert view.data_ptr() % 4 == offset
        overlay.render_device([view], [records])
        assert np.array_equal(view.cpu().numpy(), want), offset
        assert int(buf[:offset].sum()) == 0 and int(buf[offset + H * W * 3:].sum()) == 0      # nothing around it


@pytest.mark.parametrize("w", [1, 2, 3, 4, 5])
def test_boxes_at_the_image_edges(device, w):
    """a box cut by each of the four edges, one wholly outside, one covering everything, a 1 x 1 box: each alone and all
    together, plain and tinted"""
    H, W = 37, 70
    rng = np.random.default_rng(40 + w)
    boxes = [(-6, 10, 20, 25), (50, 8, 90, 30), (20, -9, 45, 6), (15, 30, 40, 60), (100, 100, 140, 120), (-50, -50, 200, 200),
             (33, 18, 33, 18), (-3, -3, W + 2, H + 2)]
    for alpha in (0, 90):
        each = [[make_record(b, (13 + 20 * k, 240 - 25 * k, 7 * k), "", thickness=w, fill_alpha=alpha)]
                for k, b in enumerate(boxes)]
        pixels = [C.background(rng, H, W) for _ in each]
        got = _check(pixels, each, device)
        assert np.array_equal(got[4], pixels[4])                           # the box outside changes nothing
        _check([C.background(rng, H, W)], [[r for records in each for r in records]], device)


def test_more_records_than_one_chunk_keep_their_order(device):
    """DEVICE_CHUNK + 22 mutually overlapping tinted, labelled records with distinct colours on 48 x 96 (two tiles): lost
    order inside a chunk or across chunks, or a pass B that does not wait for all of pass A, changes bytes"""
    n = overlay.DEVICE_CHUNK + 22
    rng = np.random.default_rng(6)
    H, W = 48, 96
    bg = C.background(rng, H, W)
    records = []
    for k in range(n):
        x0, y0 = int(rng.integers(-4, 30)), int(rng.integers(-4, 16))
        color = (k % 256, (k * 7 + k // 256) % 256, (255 - k * 3) % 256)
        records.append(make_record((x0, y0, x0 + int(rng.integers(40, 70)), y0 + int(rng.integers(24, 40))), color,
                                   "r%d" % k, thickness=1 + k % 3, fill_alpha=(64, 128)[k % 2]))
    assert len(set(r.color for r in records)) == n
    got = _check([bg], [records], device)[0]
    # the check has teeth: the same records in another order, and pass B taken per record, give other bytes
    assert not np.array_equal(got, render_host(bg, records[::-1]))
    interleaved = bg.copy()
    for r in records:
        render_host(interleaved, [r], inplace=True)
    assert not np.array_equal(got, interleaved)


def test_labels(device):
    """labels of 0, 1 and 64 characters; one running off the right edge, one at the top edge (inside its box), one partly
    below the bottom, two plates overlapping; every glyph of the table"""
    rng = np.random.default_rng(7)
    H, W = 60, 400
    every = "".join(chr(c) for c in range(0x20, 0x7f))
    records = [make_record((10, 30, 60, 50), (250, 250, 10), ""),
               make_record((70, 30, 120, 50), (10, 10, 120), "j"),
               make_record((3, 14, 395, 28), (20, 160, 60), every[:64]),
               make_record((300, 40, 390, 55), (5, 5, 5), every[64:] + " off the right edge"),
               make_record((130, 4, 200, 20), (200, 30, 30), "top edge"),
               make_record((140, 30, 200, 50), (90, 90, 255), "overlapping"),
               make_record((150, 31, 210, 52), (255, 128, 0), "plates"),
               DrawRecord(20, 70, 40, 90, (255, 255, 255), 2, 0, "below the bottom", 21, 53)]
    assert len(records[2].label) == 64 and records[4].ty == 4 + 2 + 1
    _check([C.background(rng, H, W)], [records], device)
    _check([C.background(rng, 9, 23)], [[make_record((2, 2, 20, 7), (1, 2, 3), "tiny image")]], device)


def test_batches_and_launch_count(device):
    """8 images of different sizes with record ranges of their own, one without records (its bytes stay), in ONE launch;
    nine images in two; no launch at all when no image has records"""
    from da_detect_amd import _lib

    rng = np.random.default_rng(8)
    shapes = [(9, 257), (1, 5), (40, 33), (16, 16), (3, 65), (64, 48), (7, 17), (31, 100), (20, 20)]
    pixels = [C.background(rng, *s) for s in shapes]
    lists = [C.random_records(rng, 3 + 2 * k, *s) for k, s in enumerate(shapes)]
    lists[3] = []
    calls, real_call = [], _lib.call

    def counting_call(name, *args):
        calls.append(name)
        return real_call(name, *args)

    _lib.call = counting_call
    try:
        eight = _check(pixels[:8], lists[:8], device)
        assert calls == ["dadet_overlay_batch"]
        _check(pixels, lists, device)
        assert calls == ["dadet_overlay_batch"] * 3
        _check(pixels[:2], [[], []], device)
        assert calls == ["dadet_overlay_batch"] * 3
    finally:
        _lib.call = real_call
    assert np.array_equal(eight[3], pixels[3])


def test_entry_point_status_codes(device):
    from da_detect_amd import _lib

    lib = _lib.load()
    images = torch.zeros((8, 8, 8, 3), dtype=torch.uint8, device=device)
    packed, text, _ = overlay.pack_records([[make_record((1, 1, 5, 5), (1, 2, 3), "a")]])
    rec = torch.from_numpy(packed).to(device)
    txt = torch.tensor(list(text), dtype=torch.uint8, device=device)
    gly = torch.from_numpy(_glyphs.GLYPHS.copy()).to(device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def run(n, null_image=False, count=1, rec_ptr=p(rec), dims=(8, 8)):
        items = (_lib.OverlayItem * max(n, 1))()
        for k, it in enumerate(items):
            it.image = None if null_image else images[k % 8].data_ptr()
            it.H, it.W, it.first, it.count = dims[0], dims[1], 0, count
        return lib.dadet_overlay_batch(items, n, rec_ptr, p(txt), p(gly), stream)

    assert run(0) == 0
    assert lib.dadet_overlay_batch(None, 0, None, None, None, stream) == 0
    torch.cuda.synchronize()
    assert int(images.sum()) == 0                                          # n = 0 draws nothing
    assert run(8) == 0
    assert run(9) == -1 and run(-1) == -1                                  # DADET_EINVAL
    assert run(1, null_image=True) == -1
    assert run(1, count=1025) == -1 and run(1, count=-1) == -1
    assert run(1, rec_ptr=None) == -1
    assert run(1, dims=(0, 8)) == -1 and run(1, dims=(1 << 15, 1 << 14)) == -1            # H * W above 2^28
    assert lib.dadet_overlay_batch(None, 1, p(rec), p(txt), p(gly), stream) == -1
    assert b"overlay_batch" in lib.dadet_last_error()
    torch.cuda.synchronize()
    want = render_host(np.zeros((8, 8, 3), np.uint8), [make_record((1, 1, 5, 5), (1, 2, 3), "a")])
    for k in range(8):                                                     # the refused calls drew nothing more
        assert np.array_equal(images[k].cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------------- tool, predictor
def test_tool_device_files_equal_host_files(device, tmp_path):
    from PIL import Image

    paths = C.write_coco_set(tmp_path / "set")
    tool = C.load_tool()
    common = ["--dataset", paths["spec"], "--predictions", paths["a"], "--gt", "--compare", paths["b"], "--fill-alpha", "48"]
    tool.main(common + ["--out", str(tmp_path / "host"), "--host"])
    tool.main(common + ["--out", str(tmp_path / "device")])
    names = sorted(os.listdir(str(tmp_path / "host")))
    assert names == sorted(os.listdir(str(tmp_path / "device"))) == ["frame_%d.png" % i for i in range(4)]
    for i, name in enumerate(names):
        host = np.array(Image.open(str(tmp_path / "host" / name)))
        assert np.array_equal(host, np.array(Image.open(str(tmp_path / "device" / name))))
        assert np.array_equal(host, C.expected_panels(paths, i, True, [paths["a"], paths["b"]], fill_alpha=48))


def test_coco_demo(device):
    """COCODemo on the small R-50-C4 of the golden evaluation tests, weights filled: run_on_image is render_host of the draw
    list of its own predictions, run_on_opencv_image the same with the channels reversed"""
    from da_detect_amd import _C
    from da_detect_amd.data.cityscapes import CATEGORIES
    from da_detect_amd.demo.predictor import COCODemo
    from golden.cases import case_cfg
    from golden.fill import fill_state_dict

    c = case_cfg("da_plain")
    c.merge_from_list(["MODEL.WEIGHT", ""])
    names = ("__background__",) + tuple(CATEGORIES)
    demo = COCODemo(c, confidence_threshold=0.06, min_image_size=96, categories=names)
    demo.model.load_state_dict(fill_state_dict(demo.model.state_dict(), 3))
    _C.bump_weight_epoch()
    assert demo.CATEGORIES == list(names) and COCODemo.CATEGORIES[1] == "person" and len(COCODemo.CATEGORIES) == 81
    img = C.background(np.random.default_rng(12), 120, 200)
    prediction = demo.compute_prediction(img, rgb=True)
    assert prediction.size == (200, 120) and prediction.mode == "xyxy" and prediction.bbox.device.type == "cpu"
    with torch.no_grad():                                                  # shorter side 120 -> 96: the detector sees 96 x 160
        raw = demo.model(demo.transforms(torch.from_numpy(img).to(device)))[0].to("cpu")
    assert raw.size == (160, 96) and len(raw) == len(prediction)
    assert torch.equal(prediction.bbox, raw.resize((200, 120)).bbox)       # boxes live at the image's own scale
    top = demo.select_top_predictions(prediction)
    scores = top.get_field("scores")
    assert len(top) >= 1 and bool((scores > 0.06).all()) and bool((scores[:-1] >= scores[1:]).all())
    records = overlay.build_draw_list(top, names)
    assert len(records) == len(top) and all(r.label for r in records)
    want = render_host(img, records)
    assert not np.array_equal(want, img)                                   # something is drawn
    got = demo.run_on_image(img)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(demo.run_on_opencv_image(img[:, :, ::-1]), want[:, :, ::-1])
    assert torch.equal(demo.compute_prediction(img[:, :, ::-1]).bbox, prediction.bbox)          # BGR by default
    boxes = demo.overlay_boxes(img, top, rgb=True)
    assert np.array_equal(boxes, render_host(img, overlay.boxes_only(records)))
    assert np.array_equal(demo.overlay_class_names(boxes, top, rgb=True), want)
    with pytest.raises(NotImplementedError):
        COCODemo(c, show_mask_heatmaps=True)
    masks = c.clone()
    masks.merge_from_list(["MODEL.MASK_ON", True])
    with pytest.raises(NotImplementedError):
        COCODemo(masks)
