"""Colour jitter in Pillow's 8-bit arithmetic: the numpy statement (`jitter_host`) and the device launch (`jitter_device`,
csrc/color_jitter.hip).

What is restated is torchvision's ColorJitter on its PIL back end: adjust_brightness / adjust_contrast / adjust_saturation
are Pillow's ImageEnhance.Brightness / Contrast / Color — `Image.blend(degenerate, image, factor)` with the degenerate
image black, the rounded mean grey level, the image's own `convert("L")` — and adjust_hue is `convert("HSV")`, the h plane
shifted modulo 256, `convert("RGB")`.  Every operator maps uint8 RGB to uint8 RGB; f32(.) / f64(.) below mean rounding to
float32 / float64, integer casts truncate:

  blend(d, x, a), a as float32:  a == 0 -> d;  a == 1 -> x;  else t = f32(f32(d) + f32(a * f32(x - d))) (difference in
      int), (uint8)(int)t for 0 <= a <= 1, and 0 where t <= 0, 255 where t >= 255, (uint8)(int)t elsewhere outside it
  L(r, g, b) = (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16
  brightness(f) = blend(0, x, f);  saturation(f) = blend(L, x, f);
  contrast(f) = blend(m, x, f),  m = int(sum(L) / count + 0.5) over the image as it ENTERS the operator
      ( = (2 * sum + count) // (2 * count): for count <= 2^28 the double division cannot round across a half)
  hue(f): RGB -> HSV, h = (h + int(f * 255)) mod 256 (the shift truncated toward zero first: f = -0.1 shifts by 231),
      HSV -> RGB; the round trip is not the identity, so a drawn factor of 0 still changes pixels
  RGB -> HSV: v = max, mn = min, cr = f32(max - mn); max == mn: h = s = 0; else s = clip8((int)f32(f32(cr / f32(max)) * 255)),
      rc = f32(f32(max - r) / cr) (gc, bc alike), h0 = f32(bc - gc) if r == max (tested first), f32(2.0 + f64(rc) - f64(bc))
      if g == max, f32(4.0 + f64(gc) - f64(rc)) otherwise; h1 = f32(fmod(f64(h0) / 6.0 + 1.0, 1.0)); h = clip8((int)(f64(h1) * 255.0))
  HSV -> RGB: s == 0: r = g = b = v; else in float32 hh = h * 6 / 255, i = floor(hh), fr = hh - i, fs = s / 255,
      p = rnd(v * (1 - fs)), q = rnd(v * (1 - fs * fr)), t = rnd(v * (1 - fs * (1 - fr))), rnd(y) = clip8(floor(y + 0.5)),
      (r, g, b) by i mod 6 = (v,t,p), (q,v,p), (p,v,t), (p,q,v), (t,p,v), (v,p,q)

An operator list `ops` is a sequence of (name, factor), name one of OPS, in the order the operators are applied — what
`transforms.ColorJitter.draw` returns and a device-path decision carries."""
import ctypes

import numpy as np

OPS = ("brightness", "contrast", "saturation", "hue")      # index = the DADET_JITTER_* code of include/dadet.h


def hue_shift(factor):
    """the integer added to the h plane: truncated toward zero, then modulo 256"""
    return int(factor * 255) % 256


def luma(rgb):
    c = rgb.astype(np.int64)
    return (c[..., 0] * 19595 + c[..., 1] * 38470 + c[..., 2] * 7471 + 0x8000) >> 16


def blend(degenerate, image, alpha):
    """Image.blend(degenerate, image, alpha) on uint8 arrays (degenerate broadcasts against image)"""
    a = np.float32(alpha)
    d = np.broadcast_to(np.asarray(degenerate), image.shape)
    if a == 0:
        return d.astype(np.uint8)
    if a == 1:
        return image.astype(np.uint8)
    diff = (image.astype(np.int32) - d.astype(np.int32)).astype(np.float32)
    t = d.astype(np.float32) + a * diff                    # float32 throughout: two roundings
    if 0 <= a <= 1:
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.int32))).astype(np.uint8)


def _clip8(v):
    return np.clip(v, 0, 255)


def rgb_to_hsv(rgb):
    r, g, b = (rgb[..., k].astype(np.int32) for k in range(3))
    mx, mn = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    grey = mx == mn
    cr = np.where(grey, 1, mx - mn).astype(np.float32)
    top = np.where(grey, 1, mx).astype(np.float32)
    s = _clip8(((cr / top) * np.float32(255)).astype(np.int32))
    rc, gc, bc = ((mx - c).astype(np.float32) / cr for c in (r, g, b))
    h0 = np.where(r == mx, bc - gc,
                  np.where(g == mx, (2.0 + rc.astype(np.float64) - bc.astype(np.float64)).astype(np.float32),
                           (4.0 + gc.astype(np.float64) - rc.astype(np.float64)).astype(np.float32)))
    h1 = np.fmod(h0.astype(np.float64) / 6.0 + 1.0, 1.0).astype(np.float32)
    h = _clip8((h1.astype(np.float64) * 255.0).astype(np.int32))
    return np.where(grey, 0, h), np.where(grey, 0, s), mx


def hsv_to_rgb(h, s, v):
    f = np.float32
    hh = (h * 6).astype(f) / f(255)
    i = np.floor(hh)
    fr, fs, fv = hh - i, s.astype(f) / f(255), v.astype(f)

    def rnd(y):
        return _clip8(np.floor(y + f(0.5)).astype(np.int32))

    p, q, t = rnd(fv * (f(1) - fs)), rnd(fv * (f(1) - fs * fr)), rnd(fv * (f(1) - fs * (f(1) - fr)))
    sector = i.astype(np.int32) % 6
    table = ((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q))
    out = [np.select([sector == k for k in range(6)], [table[k][c] for k in range(6)]) for c in range(3)]
    return np.stack([np.where(s == 0, v, c) for c in out], axis=-1).astype(np.uint8)


def contrast_level(rgb):
    """the one grey level of ImageEnhance.Contrast: int(mean(L) + 0.5), in integers"""
    total, count = int(luma(rgb).sum()), rgb.shape[0] * rgb.shape[1]
    return (2 * total + count) // (2 * count)


def jitter_host(pixels_u8, ops):
    """uint8 [H,W,3] RGB numpy array, ops = [(name, factor), ...] in applied order -> uint8 [H,W,3]"""
    x = np.ascontiguousarray(pixels_u8, dtype=np.uint8)
    assert x.ndim == 3 and x.shape[2] == 3
    for name, factor in ops:
        if name == "brightness":
            x = blend(np.uint8(0), x, factor)
        elif name == "contrast":
            x = blend(np.uint8(contrast_level(x)), x, factor)
        elif name == "saturation":
            x = blend(luma(x).astype(np.uint8)[..., None], x, factor)
        elif name == "hue":
            h, s, v = rgb_to_hsv(x)
            x = hsv_to_rgb((h + hue_shift(factor)) % 256, s, v)
        else:
            raise ValueError("unknown jitter operator %r (one of %s)" % (name, ", ".join(OPS)))
    return x


# ----------------------------------------------------------------------------------------------------------- the device
def jitter_device(images_u8, op_lists, sums=None):
    """images_u8: uint8 [H,W,3] device tensors; op_lists: one operator list per image -> list of tensors: a new buffer for
    every image with a non-empty list, the image itself for an empty one.  One dadet_color_jitter_batch call (a sum pass
    when any list holds the contrast, an apply pass) per _lib.JITTER_BATCH_MAX images on the current stream; none at all
    when every list is empty.  sums: int64 device tensor of at least JITTER_BATCH_MAX words to use as the scratch."""
    import torch

    from .. import _lib

    assert len(images_u8) == len(op_lists)
    out = list(images_u8)
    todo = [i for i, ops in enumerate(op_lists) if len(ops)]
    cur = None
    for first in range(0, len(todo), _lib.JITTER_BATCH_MAX):
        chunk = todo[first:first + _lib.JITTER_BATCH_MAX]
        items = (_lib.JitterItem * len(chunk))()
        keep = []
        for it, i in zip(items, chunk):
            img, ops = images_u8[i], op_lists[i]
            if not img.is_cuda:
                raise _lib.DadetError("jitter_device: the images must live on the HIP device")
            assert img.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == 3
            if len(ops) > _lib.JITTER_MAX_OPS:
                raise _lib.DadetError("jitter_device: %d operators (at most %d)" % (len(ops), _lib.JITTER_MAX_OPS))
            img = img.contiguous()
            if img.data_ptr() % 16:
                img = img.clone()                              # a view at an odd offset: the kernel loads 16 bytes at a time
            out[i] = torch.empty_like(img)
            keep += [img, out[i]]
            it.src, it.out, it.H, it.W, it.n_ops = img.data_ptr(), out[i].data_ptr(), int(img.shape[0]), int(img.shape[1]), len(ops)
            for k, (name, factor) in enumerate(ops):
                it.op[k] = OPS.index(name)
                if name == "hue":
                    it.hue_shift = hue_shift(factor)
                else:
                    it.factor[k] = float(factor)
        dev = keep[0].device
        cur = torch.cuda.current_stream(dev)
        if sums is None:
            sums = torch.empty(_lib.JITTER_BATCH_MAX, dtype=torch.int64, device=dev)
        assert sums.dtype == torch.int64 and sums.numel() >= _lib.JITTER_BATCH_MAX and sums.device == dev
        _lib.call("dadet_color_jitter_batch", items, len(chunk), ctypes.c_void_p(sums.data_ptr()),
                  ctypes.c_void_p(cur.cuda_stream))
        for t in keep + [sums]:
            t.record_stream(cur)                                 # (the pixels may come from another stream's allocation)
    return out
