"""Sample transforms — host-side API of the reference (maskrcnn_benchmark/data/transforms/transforms.py:17-97,
transforms/build.py:5-28) without torchvision: the image operations go to Pillow directly (which is what torchvision's
functional ops call for PIL images) and `ToTensor` / `Normalize` are a few lines of torch.  The training path does not
need these per-sample host transforms: `data/device_prep.py` applies the same ColorJitter -> Resize -> flips -> ToTensor
-> Normalize chain on the GPU, bit for bit; both draw their random decisions through `ColorJitter.draw` /
`Resize.get_size` / `RandomHorizontalFlip.toss` / `RandomVerticalFlip.toss` in the same order, so they are interchangeable.

Draw order per sample (the order of the steps in the chain): the jitter factors with random.uniform, one per enabled
operator in the order brightness, contrast, saturation, hue; random.shuffle of the enabled operators (the order they are
applied in); Resize.get_size; the horizontal toss; the vertical toss.  torchvision is not a dependency and its own draw
order changed between releases, so this order is the project's, modelled on the releases contemporary with the reference
and NOT pinned to any of them.  A step that is switched off is not in the chain and draws nothing."""
import collections
import random

import numpy as np
import torch

from . import color_jitter


class Compose(object):
    """chain of (image, target) -> (image, target) callables"""

    def __init__(self, transforms):
        self.transforms = list(transforms)

    def __call__(self, image, target):
        for step in self.transforms:
            image, target = step(image, target)
        return image, target

    def __repr__(self):
        return "Compose(%s)" % ", ".join(type(t).__name__ for t in self.transforms)


class Resize(object):
    """shorter side to one of `min_size` (drawn per sample), longer side capped at `max_size`"""

    def __init__(self, min_size, max_size):
        self.min_size = tuple(min_size) if isinstance(min_size, (list, tuple)) else (min_size,)
        self.max_size = max_size

    def get_size(self, image_size):
        """(w, h) -> (out_h, out_w), the arithmetic of transforms.py:41-62 (float ratio first, truncation of the
        longer side, rounding only when the cap applies) written on (short, long) instead of per orientation"""
        w, h = image_size
        short, long_ = (w, h) if w <= h else (h, w)
        goal = random.choice(self.min_size)
        if self.max_size is not None and float(long_) / float(short) * goal > self.max_size:
            goal = int(round(self.max_size * float(short) / float(long_)))
        if short == goal:
            return (h, w)
        stretched = int(goal * long_ / short)
        return (stretched, goal) if w < h else (goal, stretched)

    def __call__(self, image, target):
        from PIL import Image

        out_h, out_w = self.get_size(image.size)
        image = image.resize((out_w, out_h), Image.BILINEAR)   # what torchvision's F.resize does for a PIL image
        return image, (target.resize(image.size) if target is not None else None)


class RandomHorizontalFlip(object):
    def __init__(self, prob=0.5):
        self.prob = prob

    def toss(self):
        """one draw per sample from the global `random` stream (the device path calls this too, in the same order)"""
        return random.random() < self.prob

    def __call__(self, image, target):
        if not self.toss():
            return image, target
        from PIL import Image

        flipped = image.transpose(Image.FLIP_LEFT_RIGHT)
        return flipped, (target.transpose(0) if target is not None else None)


class RandomVerticalFlip(object):
    def __init__(self, prob=0.5):
        self.prob = prob

    def toss(self):
        """one draw per sample from the global `random` stream (the device path calls this too, in the same order)"""
        return random.random() < self.prob

    def __call__(self, image, target):
        if not self.toss():
            return image, target
        from PIL import Image

        flipped = image.transpose(Image.FLIP_TOP_BOTTOM)
        return flipped, (target.transpose(1) if target is not None else None)


class ColorJitter(object):
    """torchvision's ColorJitter on a PIL image, through Pillow itself.  A number v for brightness / contrast / saturation
    is the range [max(0, 1 - v), 1 + v], for hue [-v, v] with 0 <= v <= 0.5; a pair is the range itself.  An operator
    whose range is the single neutral value (1, for hue 0) is off: no draw, no pass over the image."""

    def __init__(self, brightness=0, contrast=0, saturation=0, hue=0):
        given = (brightness, contrast, saturation, hue)
        self.ranges = []                                         # (name, lo, hi) of the enabled operators, in draw order
        for name, value in zip(color_jitter.OPS, given):
            is_hue = name == "hue"
            if isinstance(value, (list, tuple)):
                if len(value) != 2:
                    raise ValueError("%s: a range has two ends, got %r" % (name, value))
                lo, hi = float(value[0]), float(value[1])
            else:
                if value < 0:
                    raise ValueError("%s: a single value must not be negative, got %r" % (name, value))
                lo, hi = (-float(value), float(value)) if is_hue else (max(0.0, 1.0 - value), 1.0 + value)
            bound = (-0.5, 0.5) if is_hue else (0.0, float("inf"))
            if not bound[0] <= lo <= hi <= bound[1]:
                raise ValueError("%s: range (%r, %r) outside [%r, %r]" % (name, lo, hi, bound[0], bound[1]))
            if lo == hi == (0.0 if is_hue else 1.0):
                continue
            self.ranges.append((name, lo, hi))

    def draw(self):
        """-> [(name, factor), ...] in the order the operators are applied: the factors first, then the shuffle"""
        ops = [(name, random.uniform(lo, hi)) for name, lo, hi in self.ranges]
        random.shuffle(ops)
        return ops

    @staticmethod
    def apply(image, ops):
        """ops on an RGB PIL image, by Pillow (what torchvision's functional_pil calls)"""
        from PIL import Image, ImageEnhance

        enhancers = {"brightness": ImageEnhance.Brightness, "contrast": ImageEnhance.Contrast, "saturation": ImageEnhance.Color}
        for name, factor in ops:
            if name == "hue":
                h, s, v = image.convert("HSV").split()
                shifted = (np.array(h, dtype=np.uint8).astype(np.int32) + color_jitter.hue_shift(factor)) % 256
                image = Image.merge("HSV", (Image.fromarray(shifted.astype(np.uint8)), s, v)).convert("RGB")
            else:
                image = enhancers[name](image).enhance(factor)
        return image

    def __call__(self, image, target):
        return self.apply(image, self.draw()), target


class ToTensor(object):
    """uint8 HWC image -> float CHW in [0, 1]"""

    def __call__(self, image, target):
        pixels = np.array(image, dtype=np.uint8)    # a writable copy (torch.from_numpy warns on read-only views)
        pixels = pixels[:, :, None] if pixels.ndim == 2 else pixels
        chw = torch.from_numpy(np.ascontiguousarray(pixels)).permute(2, 0, 1)
        return chw.to(torch.float32).div(255), target


class Normalize(object):
    """optionally RGB [0,1] -> BGR [0,255], then (x - mean) / std per channel"""

    def __init__(self, mean, std, to_bgr255=True):
        self.mean, self.std, self.to_bgr255 = mean, std, to_bgr255

    def __call__(self, image, target):
        x = image[[2, 1, 0]] * 255 if self.to_bgr255 else image
        shift = torch.as_tensor(self.mean, dtype=x.dtype).view(-1, 1, 1)
        scale = torch.as_tensor(self.std, dtype=x.dtype).view(-1, 1, 1)
        return (x - shift) / scale, target


def draw_decisions(transforms, image_size):
    """the random decisions `transforms` (a Compose of the steps above) would take for an image of `image_size` = (w, h),
    drawn from the same stream in the same order — per step, so Resize.get_size before the flip toss — without applying
    anything: -> ((out_h, out_w), flip) for a chain of Resize and RandomHorizontalFlip, and
    ((out_h, out_w), flip, vertical flip, jitter operators) for a chain that also holds a RandomVerticalFlip or a
    ColorJitter — the operators a tuple of (name, factor) in applied order, empty without a ColorJitter.  For the device
    path (data/device_prep.py), which applies them in its kernels; `split_decision` reads either form."""
    w, h = image_size
    size, flip, vflip, jitter, longer = (h, w), False, False, (), False
    for step in getattr(transforms, "transforms", ()):
        if isinstance(step, Resize):
            size = step.get_size((size[1], size[0]))
        elif isinstance(step, RandomHorizontalFlip):
            flip = step.toss() != flip
        elif isinstance(step, RandomVerticalFlip):
            vflip, longer = step.toss() != vflip, True
        elif isinstance(step, ColorJitter):
            jitter, longer = jitter + tuple(step.draw()), True
    if longer:
        return (int(size[0]), int(size[1])), bool(flip), bool(vflip), jitter
    return (int(size[0]), int(size[1])), bool(flip)


def split_decision(decision):
    """a decision of `draw_decisions`, short or long -> ((out_h, out_w), flip, vertical flip, jitter operators)"""
    if len(decision) == 2:
        return decision[0], decision[1], False, ()
    size, flip, vflip, jitter = decision
    return size, flip, vflip, jitter


TransformParams = collections.namedtuple("TransformParams", ["min_size", "max_size", "flip_prob", "vertical_flip_prob", "jitter"])


def transform_params(cfg, is_train=True):
    """what transforms/build.py:5-23 reads from the configuration; jitter = (brightness, contrast, saturation, hue).
    Test-time transforms get neither jitter nor flips."""
    if is_train:
        i = cfg.INPUT
        return TransformParams(i.MIN_SIZE_TRAIN, i.MAX_SIZE_TRAIN, i.HORIZONTAL_FLIP_PROB_TRAIN, i.VERTICAL_FLIP_PROB_TRAIN,
                               (i.BRIGHTNESS, i.CONTRAST, i.SATURATION, i.HUE))
    return TransformParams(cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST, 0, 0, (0, 0, 0, 0))


def build_transforms(cfg, is_train=True):
    """ColorJitter -> Resize -> RandomHorizontalFlip -> RandomVerticalFlip -> ToTensor -> Normalize (transforms/build.py:36-45);
    a jitter with no operator on and a vertical flip of probability 0 are left out — the reference's main tree, which this
    port follows, has neither step, so they must not draw"""
    p = transform_params(cfg, is_train)
    jitter = ColorJitter(*p.jitter)
    steps = [jitter] if jitter.ranges else []
    steps += [Resize(p.min_size, p.max_size), RandomHorizontalFlip(p.flip_prob)]
    if p.vertical_flip_prob > 0:
        steps.append(RandomVerticalFlip(p.vertical_flip_prob))
    steps += [ToTensor(), Normalize(mean=cfg.INPUT.PIXEL_MEAN, std=cfg.INPUT.PIXEL_STD, to_bgr255=cfg.INPUT.TO_BGR255)]
    return Compose(steps)
