"""Colour jitter and vertical flip on the host: data/color_jitter.py jitter_host (the numpy statement of Pillow's 8-bit
arithmetic, which the device kernel is held to in test_color_jitter_gpu.py) against Pillow itself, the ColorJitter /
RandomVerticalFlip steps of data/transforms.py, the draw order shared by the host chain and draw_decisions, the six INPUT
keys, and the default chain staying what it was."""
import itertools
import random

import numpy as np
import pytest
import torch

pytest.importorskip("PIL")
from PIL import Image, ImageEnhance  # noqa: E402

from da_detect_amd.data import color_jitter as CJ  # noqa: E402
from da_detect_amd.data import transforms as T  # noqa: E402

ENHANCE = {"brightness": ImageEnhance.Brightness, "contrast": ImageEnhance.Contrast, "saturation": ImageEnhance.Color}
_CACHE = {}


def all_colours():
    """the 4096 x 4096 image of all 2^24 colours (built once, never modified)"""
    if "all" not in _CACHE:
        v = np.arange(1 << 24, dtype=np.uint32)
        img = np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)
        img.setflags(write=False)
        _CACHE["all"] = img
    return _CACHE["all"]


def pillow_op(pixels, name, factor):
    """one operator by Pillow, the way torchvision's functional_pil calls it"""
    image = Image.fromarray(pixels)
    if name != "hue":
        return np.asarray(ENHANCE[name](image).enhance(factor))
    h, s, v = image.convert("HSV").split()
    shifted = ((np.asarray(h).astype(np.int32) + int(factor * 255)) % 256).astype(np.uint8)
    return np.asarray(Image.merge("HSV", (Image.fromarray(shifted), s, v)).convert("RGB"))


@pytest.mark.parametrize("factor", [0.0, 0.3, -0.1])
def test_hue_on_all_colours(factor):
    """shifts 0 (the round trip alone: not the identity), 76 and 231 (-0.1 truncates to -25, then modulo 256)"""
    assert CJ.hue_shift(factor) == {0.0: 0, 0.3: 76, -0.1: 231}[factor]
    got = CJ.jitter_host(all_colours(), [("hue", factor)])
    assert np.array_equal(got, pillow_op(all_colours(), "hue", factor))
    if factor == 0.0:
        assert not np.array_equal(got, all_colours())


@pytest.mark.parametrize("factor", [0.0, 1.0, 0.37, 1.7, 2.6])
def test_brightness_and_saturation_on_all_colours(factor):
    for name in ("brightness", "saturation"):
        got = CJ.jitter_host(all_colours(), [(name, factor)])
        assert np.array_equal(got, pillow_op(all_colours(), name, factor)), name


@pytest.mark.parametrize("factor", [0.0, 1.0, 0.37, 1.7, 2.6])
def test_contrast_blend_factors(factor):
    """a 256 x 256 x 3 image in which every channel value meets the grey level (here 128) at every blend factor"""
    ramp = np.arange(256, dtype=np.uint8)
    img = np.stack([np.tile(ramp, (256, 1)), np.tile(ramp[:, None], (1, 256)), np.tile(ramp[::-1], (256, 1))], axis=-1)
    got = CJ.jitter_host(img, [("contrast", factor)])
    assert np.array_equal(got, pillow_op(img, "contrast", factor))


def test_contrast_mean_at_a_half_and_one_pixel_below():
    """grey images (L = the value): 8 pixels, four at 100 and four at 101 -> mean 100.5 exactly, m = 101; one pixel lowered
    by one level -> mean 100.375, m = 100"""
    values = np.array([100, 100, 100, 100, 101, 101, 101, 101], dtype=np.uint8).reshape(2, 4)
    img = np.repeat(values[:, :, None], 3, axis=2)
    assert CJ.contrast_level(img) == 101
    below = img.copy()
    below[1, 3] = 100
    assert CJ.contrast_level(below) == 100
    for pixels in (img, below):
        for factor in (0.0, 0.5, 1.6):
            assert np.array_equal(CJ.jitter_host(pixels, [("contrast", factor)]), pillow_op(pixels, "contrast", factor))


def test_chain_in_all_24_orders():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    factors = {"brightness": 1.23, "contrast": 0.61, "saturation": 1.48, "hue": -0.07}
    for order in itertools.permutations(CJ.OPS):
        ops = [(name, factors[name]) for name in order]
        want = img
        for name, factor in ops:
            want = pillow_op(want, name, factor)
        assert np.array_equal(CJ.jitter_host(img, ops), want), order


def test_color_jitter_step_equals_jitter_host_of_its_draw():
    rng = np.random.default_rng(6)
    img = rng.integers(0, 256, (31, 45, 3), dtype=np.uint8)
    step = T.ColorJitter(0.4, 0.4, 0.4, 0.1)
    assert [r[0] for r in step.ranges] == list(CJ.OPS)
    assert step.ranges[0][1:] == (0.6, 1.4) and step.ranges[3][1:] == (-0.1, 0.1)
    orders = set()
    for seed in range(6):
        random.seed(seed)
        ops = step.draw()
        orders.add(tuple(name for name, _ in ops))
        assert sorted(name for name, _ in ops) == sorted(CJ.OPS)
        random.seed(seed)
        out, target = step(Image.fromarray(img), None)
        assert target is None and np.array_equal(np.asarray(out), CJ.jitter_host(img, ops)), seed
    assert len(orders) > 1                                           # the shuffle mattered
    # ranges: a pair is the range itself; the neutral value switches an operator off; bad values are refused
    assert T.ColorJitter(0, (0.5, 2.0), 0, 0).ranges == [("contrast", 0.5, 2.0)]
    assert T.ColorJitter(0, (1, 1), 0, (0, 0)).ranges == []
    assert T.ColorJitter(2.0, 0, 0, 0).ranges == [("brightness", 0.0, 3.0)]
    for bad in ({"hue": 0.6}, {"brightness": -0.1}, {"hue": (-0.6, 0.1)}, {"contrast": (1.2, 0.8)}):
        with pytest.raises(ValueError):
            T.ColorJitter(**bad)


def _chain(jitter, vertical):
    steps = [T.ColorJitter(0.3, 0.2, 0.5, 0.05)] if jitter else []
    steps += [T.Resize((20, 24, 28), 60), T.RandomHorizontalFlip(0.5)]
    steps += [T.RandomVerticalFlip(0.5)] if vertical else []
    return T.Compose(steps + [T.ToTensor(), T.Normalize([1.0, 2.0, 3.0], [1.0, 1.0, 1.0])])


@pytest.mark.parametrize("jitter,vertical", [(False, False), (True, False), (False, True), (True, True)])
def test_device_decisions_consume_the_stream_like_the_host_chain(jitter, vertical):
    """same seed: draw_decisions and the host chain leave `random` in the same state, and the decisions are the ones the
    host chain applied (its output is the oracle-free restatement: jitter_host, Pillow resize, numpy flips)"""
    rng = np.random.default_rng(8)
    img = rng.integers(0, 256, (30, 50, 3), dtype=np.uint8)
    chain = _chain(jitter, vertical)
    for seed in range(8):
        random.seed(seed)
        decision = T.draw_decisions(chain, (50, 30))
        state = random.getstate()
        random.seed(seed)
        host, _ = chain(Image.fromarray(img), None)
        assert random.getstate() == state
        assert len(decision) == (4 if jitter or vertical else 2)
        (oh, ow), flip, vflip, ops = T.split_decision(decision)
        assert (not vflip or vertical) and (len(ops) == 4 if jitter else ops == ())
        want = np.asarray(Image.fromarray(CJ.jitter_host(img, ops)).resize((ow, oh), Image.BILINEAR))
        want = want[:, ::-1] if flip else want
        want = want[::-1] if vflip else want
        want, _ = T.Normalize([1.0, 2.0, 3.0], [1.0, 1.0, 1.0])(T.ToTensor()(Image.fromarray(np.ascontiguousarray(want)), None)[0], None)
        assert torch.equal(host, want), seed


def test_default_keys_build_todays_chain():
    from da_detect_amd.config import cfg
    from da_detect_amd.data.datasets import RainImage

    c = cfg.clone()
    i = c.INPUT
    assert (i.BRIGHTNESS, i.CONTRAST, i.SATURATION, i.HUE) == (0.0, 0.0, 0.0, 0.0)
    assert (i.HORIZONTAL_FLIP_PROB_TRAIN, i.VERTICAL_FLIP_PROB_TRAIN) == (0.5, 0.0)
    chain = T.build_transforms(c, True)
    assert [type(s) for s in chain.transforms] == [T.Resize, T.RandomHorizontalFlip, T.ToTensor, T.Normalize]
    assert chain.transforms[1].prob == 0.5
    # the first decisions after a seed: one choice among MIN_SIZE_TRAIN, one toss — nothing else is drawn
    c.merge_from_list(["INPUT.MIN_SIZE_TRAIN", (600, 640, 680), "INPUT.MAX_SIZE_TRAIN", 1400])
    chain = T.build_transforms(c, True)
    random.seed(11)
    got = [T.draw_decisions(chain, (2048, 1024)) for _ in range(5)]
    random.seed(11)
    want = []
    for _ in range(5):
        goal = random.choice((600, 640, 680))
        want.append(((goal, 2 * goal), random.random() < 0.5))
    assert got == want and all(len(d) == 2 for d in got)
    # all six keys set: the full chain at training time, none of it at test time
    c.merge_from_list(["INPUT.BRIGHTNESS", 0.2, "INPUT.CONTRAST", 0.2, "INPUT.SATURATION", 0.2, "INPUT.HUE", 0.05,
                       "INPUT.HORIZONTAL_FLIP_PROB_TRAIN", 0.25, "INPUT.VERTICAL_FLIP_PROB_TRAIN", 0.4])
    chain = T.build_transforms(c, True)
    assert [type(s) for s in chain.transforms] == [T.ColorJitter, T.Resize, T.RandomHorizontalFlip, T.RandomVerticalFlip,
                                                   T.ToTensor, T.Normalize]
    assert chain.transforms[2].prob == 0.25 and chain.transforms[3].prob == 0.4
    test_chain = T.build_transforms(c, False)
    assert [type(s) for s in test_chain.transforms] == [T.Resize, T.RandomHorizontalFlip, T.ToTensor, T.Normalize]
    assert test_chain.transforms[1].prob == 0
    # a rainy raw sample carries the long decision like any other
    decision = T.draw_decisions(chain, (64, 32))
    assert RainImage(torch.zeros(32, 64, 3, dtype=torch.uint8), decision, 0, None).decision == decision and len(decision) == 4


def test_upstream_yaml_with_the_six_keys_merges(tmp_path):
    from da_detect_amd.config import cfg

    path = tmp_path / "jitter.yaml"
    path.write_text("INPUT:\n  MIN_SIZE_TRAIN: (600,)\n  MAX_SIZE_TRAIN: 1200\n  BRIGHTNESS: 0.4\n  CONTRAST: 0.3\n"
                    "  SATURATION: 0.2\n  HUE: 0.1\n  HORIZONTAL_FLIP_PROB_TRAIN: 0.5\n  VERTICAL_FLIP_PROB_TRAIN: 0\n")
    c = cfg.clone()
    c.merge_from_file(str(path))
    assert (c.INPUT.BRIGHTNESS, c.INPUT.CONTRAST, c.INPUT.SATURATION, c.INPUT.HUE) == (0.4, 0.3, 0.2, 0.1)
    assert c.INPUT.VERTICAL_FLIP_PROB_TRAIN == 0.0 and isinstance(c.INPUT.VERTICAL_FLIP_PROB_TRAIN, float)
    p = T.transform_params(c, True)
    assert p.jitter == (0.4, 0.3, 0.2, 0.1) and p.flip_prob == 0.5 and p.vertical_flip_prob == 0.0
    assert T.transform_params(c, False).jitter == (0, 0, 0, 0)


def test_vertical_flip_step():
    from da_detect_amd.structures.bounding_box import BoxList

    rng = np.random.default_rng(9)
    img = Image.fromarray(rng.integers(0, 256, (21, 34, 3), dtype=np.uint8))
    boxes = BoxList(torch.tensor([[3.0, 2.0, 20.0, 9.0], [0.0, 0.0, 33.0, 20.0]]), img.size, mode="xyxy")
    out, target = T.RandomVerticalFlip(1.0)(img, boxes)
    assert np.array_equal(np.asarray(out), np.asarray(img.transpose(Image.FLIP_TOP_BOTTOM)))
    assert torch.equal(target.bbox, boxes.transpose(1).bbox) and target.bbox.tolist()[0] == [3.0, 12.0, 20.0, 19.0]
    out, target = T.RandomVerticalFlip(0.0)(img, boxes)
    assert out is img and target is boxes
    random.seed(2)
    tosses = [T.RandomVerticalFlip(0.5).toss() for _ in range(6)]
    random.seed(2)
    assert tosses == [random.random() < 0.5 for _ in range(6)] and len(set(tosses)) == 2
