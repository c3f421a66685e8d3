"""Colour jitter and vertical flip on the GPU: csrc/color_jitter.hip (dadet_color_jitter_batch: a sum pass for the contrast,
an apply pass, groups of 16 pixels with a byte-wise tail) against data/color_jitter.py jitter_host and against Pillow, bit
for bit; the flip mask of dadet_image_prepare_batch against the host chain; the device_prep loaders with all six INPUT keys
set against the host loaders."""
import random

import numpy as np
import pytest
import torch

from test_color_jitter_host import all_colours, pillow_op
from test_data_pipeline import _image
from test_device_input_gpu import TILE_H, TILE_W, _cfg, _same_field, _specs
from test_rain_host import rain_cfg, rain_specs

pytest.importorskip("PIL")
from PIL import Image  # noqa: E402

from da_detect_amd.data import color_jitter as CJ  # noqa: E402

pytestmark = pytest.mark.gpu

B, C, S, H = (("brightness", 1.31), ("contrast", 0.58), ("saturation", 1.62), ("hue", -0.13))
# every operator alone; chains of 2, 3 and 4 with the contrast first, in the middle and last
OP_LISTS = [[B], [C], [S], [H], [("brightness", 0.42)], [("contrast", 1.9)], [("saturation", 0.0)], [("hue", 0.0)],
            [C, S], [B, C],
            [C, B, H], [H, C, S], [S, H, C],
            [C, B, S, H], [B, C, H, S], [S, B, C, H], [H, S, B, C]]
SIZES = [(1, 1), (1, 5), (3, 15), (2, 16), (7, 17), (5, 63), (4, 64), (3, 65), (9, 257)]


def _device_jitter(pixels, op_lists, device, sums=None):
    """numpy images -> numpy results of ONE jitter_device call over all of them (chunks of 8 inside)"""
    on_device = [torch.from_numpy(np.ascontiguousarray(p)).to(device) for p in pixels]
    out = CJ.jitter_device(on_device, op_lists, sums)
    torch.cuda.synchronize()
    for src, p in zip(on_device, pixels):
        assert torch.equal(src.cpu(), torch.from_numpy(np.ascontiguousarray(p)))       # out is a buffer of its own
    return out


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_operators_and_chains_equal_jitter_host(device, size):
    img = _image(np.random.default_rng(size[0] * 1000 + size[1]), *size)
    got = _device_jitter([img] * len(OP_LISTS), OP_LISTS, device)
    for ops, g in zip(OP_LISTS, got):
        assert torch.equal(g.cpu(), torch.from_numpy(CJ.jitter_host(img, ops))), ops


def test_all_colours_against_pillow(device):
    """hue shifts 0 and 231 and saturation 1.7 on the 4096 x 4096 image of all 2^24 colours, against Pillow itself"""
    img = all_colours()
    cases = [("hue", 0.0), ("hue", -0.1), ("saturation", 1.7)]
    assert CJ.hue_shift(-0.1) == 231
    src = torch.from_numpy(np.array(img)).to(device)
    for name, factor in cases:
        got = CJ.jitter_device([src], [[(name, factor)]])[0]
        assert torch.equal(got.cpu(), torch.from_numpy(np.array(pillow_op(img, name, factor)))), (name, factor)


def test_contrast_sum_past_32_bits(device):
    """4112 x 4099 pixels of 255: sum(L) = 4.298e9 > 2^32.  m = 255 and the image stays white; a sum wrapped at 32 bits
    would give m = 0 and 127 everywhere.  (jitter_host of a small white image: the mean does not depend on the size.)"""
    src = torch.full((4112, 4099, 3), 255, dtype=torch.uint8, device=device)
    assert 4112 * 4099 * 255 > 1 << 32
    got = CJ.jitter_device([src], [[("contrast", 0.5)]])[0]
    want = CJ.jitter_host(np.full((4, 4, 3), 255, np.uint8), [("contrast", 0.5)])
    assert want.min() == 255 and got.shape == src.shape and int(got.min()) == 255


def test_batch_of_eight_and_reused_sums(device):
    """8 descriptors of mixed sizes and lists in ONE call — some without contrast, one empty — equal their single-image
    results; the sums scratch is handed in dirty and reused by a second call"""
    from da_detect_amd import _lib

    rng = np.random.default_rng(21)
    shapes = [(9, 257), (1, 5), (40, 33), (16, 16), (3, 65), (64, 48), (7, 17), (31, 100)]
    lists = [[C, B, S, H], [B], [H, S], [], [S, H, C], [C], [H], [B, C]]
    imgs = [_image(rng, *s) for s in shapes]
    singles = [_device_jitter([im], [ops], device)[0].cpu() for im, ops in zip(imgs, lists)]
    sums = torch.full((_lib.JITTER_BATCH_MAX,), -7, dtype=torch.int64, device=device)
    calls, real_call = [], _lib.call

    def counting_call(name, *args):
        calls.append(name)
        return real_call(name, *args)

    _lib.call = counting_call
    try:
        first = _device_jitter(imgs, lists, device, sums)
        second = _device_jitter(imgs[::-1], lists[::-1], device, sums)[::-1]
        nothing = CJ.jitter_device([torch.from_numpy(imgs[0]).to(device)], [[]])
    finally:
        _lib.call = real_call
    assert calls == ["dadet_color_jitter_batch"] * 2                 # (none for the list of empty lists)
    for k, (im, ops) in enumerate(zip(imgs, lists)):
        want = torch.from_numpy(CJ.jitter_host(im, ops))
        assert torch.equal(singles[k], want) and torch.equal(first[k].cpu(), want) and torch.equal(second[k].cpu(), want), k
    assert torch.equal(nothing[0].cpu(), torch.from_numpy(imgs[0]))
    # the contrast images' sums, in the order of the second call (reversed): B,C / C / S,H,C / C,B,S,H
    want_sums = [int(CJ.luma(CJ.jitter_host(imgs[k], lists[k][:[n for n, _ in lists[k]].index("contrast")])).sum())
                 for k in (7, 5, 4, 0)]
    assert sums[:4].tolist() == want_sums


def test_bad_jitter_descriptors_are_refused(device):
    from da_detect_amd import _lib

    img = torch.zeros((4, 4, 3), dtype=torch.uint8, device=device)
    with pytest.raises(_lib.DadetError, match="twice"):
        CJ.jitter_device([img], [[B, ("brightness", 0.5)]])
    with pytest.raises(_lib.DadetError, match="not finite"):
        CJ.jitter_device([img], [[("contrast", float("nan"))]])
    with pytest.raises(_lib.DadetError):
        CJ.jitter_device([img.cpu()], [[B]])


@pytest.mark.parametrize("mask", [0, 1, 2, 3])
def test_flip_mask_against_the_host_chain(device, mask):
    """out_h in {T, T + 1} x out_w in {Tw, Tw + 1} for the 16 x 64 tile in one launch of four: Pillow resize, the two
    transposes, ToTensor, Normalize on the host against dadet_image_prepare_batch with the flip mask, padding included"""
    from da_detect_amd.data import device_prep as P
    from da_detect_amd.data import transforms as T

    c = _cfg("DATALOADER.SIZE_DIVISIBILITY", 32)
    rng = np.random.default_rng(13)
    imgs = [_image(rng, 23, 90) for _ in range(4)]
    flip, vflip = bool(mask & 1), bool(mask & 2)
    decisions = [((oh, ow), flip, vflip, ()) for oh in (TILE_H, TILE_H + 1) for ow in (TILE_W, TILE_W + 1)]
    batch = torch.full((4, 3, 32, 96), float("nan"), device=device).contiguous(memory_format=torch.channels_last)
    P.prepare_batch_into([torch.from_numpy(i).to(device) for i in imgs], decisions, c.INPUT.PIXEL_MEAN, c.INPUT.PIXEL_STD,
                         c.INPUT.TO_BGR255, batch)
    got = batch.cpu()
    normalize = T.Normalize(c.INPUT.PIXEL_MEAN, c.INPUT.PIXEL_STD, c.INPUT.TO_BGR255)
    for i, (im, ((oh, ow), _, _, _)) in enumerate(zip(imgs, decisions)):
        pil = Image.fromarray(im).resize((ow, oh), Image.BILINEAR)
        pil = pil.transpose(Image.FLIP_LEFT_RIGHT) if flip else pil
        pil = pil.transpose(Image.FLIP_TOP_BOTTOM) if vflip else pil
        want, _ = normalize(T.ToTensor()(pil, None)[0], None)
        assert torch.equal(got[i, :, :oh, :ow], want), (i, mask)
        assert not got[i, :, oh:, :].any() and not got[i, :, :, ow:].any()       # (NaN left behind fails this too)
    # the single-image entry takes the same mask
    slot = torch.zeros((1, 3, 17, 65), device=device).contiguous(memory_format=torch.channels_last)
    P.resize_normalize_into(torch.from_numpy(imgs[3]).to(device), (17, 65), mask, c.INPUT.PIXEL_MEAN, c.INPUT.PIXEL_STD,
                            c.INPUT.TO_BGR255, slot[0])
    assert torch.equal(slot[0].cpu(), got[3, :, :17, :65])


def test_da_loaders_with_all_six_keys_equal_the_host_loaders(device, tmp_path):
    """make_da_data_loaders with and without device_prep under jitter, both flips and a size draw: images and boxes"""
    from da_detect_amd.data.build import make_da_data_loaders

    specs = _specs(tmp_path, ("source", "target"))
    c = _cfg("SOLVER.IMS_PER_BATCH", 4, "SOLVER.MAX_ITER", 2, "DATALOADER.NUM_WORKERS", 0, "DATALOADER.SIZE_DIVISIBILITY", 32,
             "INPUT.MIN_SIZE_TRAIN", (96, 80), "INPUT.MAX_SIZE_TRAIN", 192, "MODEL.DOMAIN_ADAPTATION_ON", True,
             "INPUT.BRIGHTNESS", 0.4, "INPUT.CONTRAST", 0.4, "INPUT.SATURATION", 0.4, "INPUT.HUE", 0.1,
             "INPUT.HORIZONTAL_FLIP_PROB_TRAIN", 0.5, "INPUT.VERTICAL_FLIP_PROB_TRAIN", 0.5)
    collected = {}
    for device_prep in (False, True):
        torch.manual_seed(9)
        random.seed(3)
        collected[device_prep] = list(zip(*make_da_data_loaders(c, specs, device_prep=device_prep)))
    torch.cuda.synchronize()
    assert len(collected[True]) == len(collected[False]) == 2
    for got_step, want_step in zip(collected[True], collected[False]):
        for got, want in zip(got_step, want_step):              # per domain: (ImageList, targets, ids)
            assert len(got) == len(want) == 3
            for g, w in zip(got, want):
                _same_field(g, w)
    # the keys mattered: the same seed without them gives other pixels
    torch.manual_seed(9)
    random.seed(3)
    plain = _cfg("SOLVER.IMS_PER_BATCH", 4, "SOLVER.MAX_ITER", 2, "DATALOADER.NUM_WORKERS", 0, "DATALOADER.SIZE_DIVISIBILITY", 32,
                 "INPUT.MIN_SIZE_TRAIN", (96, 80), "INPUT.MAX_SIZE_TRAIN", 192, "MODEL.DOMAIN_ADAPTATION_ON", True)
    first = next(iter(make_da_data_loaders(plain, specs)[0]))
    want = collected[False][0][0][0].tensors
    assert first[0].tensors.shape != want.shape or not torch.equal(first[0].tensors, want)


def test_aligned_rain_triplet_with_jitter_equals_the_host_loader(device, tmp_path):
    """the aligned triplet with a synthesised rainy domain: the rainy sample shares the source sample's upload, is
    synthesised first and jittered as a rainy image with its own draw — as on the host chain"""
    from da_detect_amd.data.build import make_triplet_data_loader

    specs = rain_specs(tmp_path)
    c = rain_cfg("SOLVER.MAX_ITER", 2, "INPUT.BRIGHTNESS", 0.3, "INPUT.CONTRAST", 0.3, "INPUT.SATURATION", 0.3, "INPUT.HUE", 0.05,
                 "INPUT.VERTICAL_FLIP_PROB_TRAIN", 0.5)
    collected = {}
    for device_prep in (False, True):
        torch.manual_seed(9)
        random.seed(3)
        collected[device_prep] = list(make_triplet_data_loader(c, specs, device_prep=device_prep))
    torch.cuda.synchronize()
    assert len(collected[True]) == len(collected[False]) == 2
    for got, want in zip(collected[True], collected[False]):
        assert len(got) == len(want) == 9
        for g, w in zip(got, want):
            _same_field(g, w)
