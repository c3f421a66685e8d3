"""The auxiliary rainy domain, synthesised instead of rendered offline (reference: efficientderain-master/
generate_rainy_cityscape.py rain_aug, augment_and_mix.py augment_and_mix(layer, severity=3, width=3, depth=-1),
augmentations.py rotate / shear_x / shear_y / translate_x / translate_y / zoom_x / zoom_y).

A rainy image is the screen blend of the source pixels with a rain layer R: the rain-mask image mixed with three chains
of affine warps of itself.  `draw_rain_plan` makes the reference's draws from a numpy RandomState, in its order, and
turns every operator into the six numbers Pillow's Image.transform(size, AFFINE, data, BILINEAR) receives; applying a
plan is deterministic.  `synthesize_host` applies it with Pillow and numpy (the CPU path of the host transform chain
and the tests' oracle), `synthesize_device` with csrc/rain.hip (dadet_rain_synthesize), bit for bit the same.

On purpose not the reference's: masks are read with Pillow and brought to the image's size with Image.resize(BILINEAR)
(the reference: cv2.resize), cached per (mask, size); the mask index is drawn from Python's `random` like the other
per-sample decisions; the two randint draws whose results the reference never uses are not made; every sample seeds its
own RandomState with random.getrandbits(32), so inside the DataLoader worker under that worker's seeding.  The 8-bit
rounding of the composite (half to even, saturated) is what OpenCV documents for imwrite of a float image
(saturate_cast / cvRound); OpenCV was not available to pin it."""
import collections
import ctypes
import math
import os

import numpy as np

OPERATORS = ("rotate", "shear_x", "shear_y", "translate_x", "translate_y", "zoom_x", "zoom_y")
SEVERITY = 3
WIDTH = 3
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)

# ws float32 [3]; c0, c1 float32; depth; coeffs float64 [3][depth][6]; ops [3][depth] of (operator name, parameter)
RainPlan = collections.namedtuple("RainPlan", ["ws", "c0", "c1", "depth", "coeffs", "ops"])


def rotate_coeffs(degrees, W, H):
    """the matrix of Pillow's Image.rotate(degrees, BILINEAR) about (W / 2, H / 2); 0 degrees is a copy there, and the
    identity data here (the bilinear warp of the identity returns its input)"""
    angle = degrees % 360.0
    if angle == 0:
        return IDENTITY
    angle = -math.radians(angle)
    a, b = round(math.cos(angle), 15), round(math.sin(angle), 15)
    d, e = round(-math.sin(angle), 15), round(math.cos(angle), 15)
    cx, cy = W / 2, H / 2
    c = a * -cx + b * -cy + 0.0
    f = d * -cx + e * -cy + 0.0
    return (a, b, c + cx, d, e, f + cy)


def operator_coeffs(name, level, toss, W, H):
    """one operator of augmentations.py -> (AFFINE data, the parameter it derived); level = its uniform(0.1, 3) draw,
    toss = its sign / side draw"""
    if name == "rotate":
        degrees = int(level * 30 / 10)
        degrees = -degrees if toss > 0.5 else degrees
        return rotate_coeffs(degrees, W, H), degrees
    if name in ("shear_x", "shear_y"):
        s = float(level) * 0.3 / 10.
        s = -s if toss > 0.5 else s
        return ((1, s, 0, 0, 1, 0) if name == "shear_x" else (1, 0, 0, s, 1, 0)), s
    if name in ("translate_x", "translate_y"):
        t = int(level * ((W if name == "translate_x" else H) / 3) / 10)
        t = -t if toss > 0.5 else t
        return ((1, 0, t, 0, 1, 0) if name == "translate_x" else (1, 0, 0, 0, 1, t)), t
    if name in ("zoom_x", "zoom_y"):
        rate = 1.0 / (float(level) * 6.0 / 10.)
        size = W if name == "zoom_x" else H
        bias = size * (1 - rate) if toss > 0.5 else 0
        return ((rate, 0, bias, 0, 1, 0) if name == "zoom_x" else (1, 0, 0, 0, rate, bias)), rate
    raise ValueError(name)


def make_plan(ws, m, chains):
    """ws: the three chain weights, m: the mixing draw, chains: per chain a list of (name, parameter, AFFINE data) — all
    of one depth"""
    ws = np.asarray(ws, dtype=np.float32)
    m = np.float32(m)
    depth = len(chains[0])
    assert len(chains) == WIDTH and all(len(c) == depth for c in chains) and depth >= 1
    c0 = np.float32(max(np.float32(1) - m, 0.7))
    c1 = np.float32(max(m, (np.float32(1.0) / max(ws)) * np.float32(0.5)))
    coeffs = np.array([[[float(v) for v in op[2]] for op in chain] for chain in chains], dtype=np.float64)
    return RainPlan(ws, c0, c1, depth, coeffs, [[(op[0], op[1]) for op in chain] for chain in chains])


def draw_rain_plan(rs, W, H):
    """augment_and_mix's draws from the RandomState `rs` for a W x H layer: dirichlet, beta, ONE depth (the reference
    reassigns `depth` in its first chain, so the later chains inherit it), then per chain and operator: the choice, the
    level, the toss (uniform() for rotate and the shears, random_sample() for the translates and zooms — one stream)"""
    ws = np.float32(rs.dirichlet([1.0] * WIDTH))
    m = np.float32(rs.beta(1.0, 1.0))
    depth = int(rs.randint(2, 4))
    chains = []
    for _ in range(WIDTH):
        chain = []
        for _ in range(depth):
            name = OPERATORS[int(rs.choice(len(OPERATORS)))]
            level = rs.uniform(low=0.1, high=SEVERITY)
            toss = rs.uniform() if name in ("rotate", "shear_x", "shear_y") else rs.random_sample()
            data, param = operator_coeffs(name, level, toss, W, H)
            chain.append((name, param, data))
        chains.append(chain)
    return make_plan(ws, m, chains)


# ------------------------------------------------------------------------------------------------------ host
def warp_numpy(image_u8, data):
    """Pillow's Geometry.c bilinear affine (affine_transform + bilinear_filter32RGB) restated in float64 numpy: pixel
    centres at +0.5, 0 outside the image, clamped neighbours, truncation to 8 bits"""
    H, W = image_u8.shape[:2]
    a = [float(v) for v in data]
    x = np.arange(W, dtype=np.float64)[None, :] + 0.5
    y = np.arange(H, dtype=np.float64)[:, None] + 0.5
    xin = (a[0] * x + a[1] * y) + a[2]
    yin = (a[3] * x + a[4] * y) + a[5]
    inside = (xin >= 0.0) & (xin < W) & (yin >= 0.0) & (yin < H)
    xin = np.where(inside, xin, 0.5) - 0.5
    yin = np.where(inside, yin, 0.5) - 0.5
    xf = np.floor(xin).astype(np.int64)
    yf = np.floor(yin).astype(np.int64)
    dx = (xin - xf)[..., None]
    dy = (yin - yf)[..., None]
    x0, x1 = np.clip(xf, 0, W - 1), np.clip(xf + 1, 0, W - 1)
    y0, y1 = np.clip(yf, 0, H - 1), np.clip(yf + 1, 0, H - 1)
    src = image_u8.astype(np.int64)
    p0, p1 = src[y0, x0], src[y0, x1]
    v1 = p0 + (p1 - p0) * dx
    q0, q1 = src[y1, x0], src[y1, x1]
    v2 = np.where((yf + 1 < H)[..., None], q0 + (q1 - q0) * dx, v1)
    v = v1 + (v2 - v1) * dy
    return np.where(inside[..., None], v, 0.0).astype(np.uint8)


def warp_pillow(image_u8, data):
    from PIL import Image

    H, W = image_u8.shape[:2]
    out = Image.fromarray(image_u8).transform((W, H), Image.AFFINE, tuple(float(v) for v in data), resample=Image.BILINEAR)
    return np.asarray(out)


def mix_host(mask_u8, plan, warp=warp_pillow):
    """the rain layer R (float32 [H,W,3], may exceed 1) — augment_and_mix's return value for the layer float32(mask) / 255,
    in numpy's evaluation order"""
    layer = mask_u8.astype(np.float32) / np.float32(255.0)
    mix = np.zeros_like(layer)
    for i in range(WIDTH):
        u = mask_u8
        for data in plan.coeffs[i]:
            u = warp(u, data)
        mix = (mix.astype(np.float64) + np.float64(plan.ws[i]) * (u / 255.)).astype(np.float32)
    return np.float32(plan.c0) * layer + np.float32(plan.c1) * mix


def composite_host(image_u8, R):
    """rain_aug's screen blend in float32 and the 8-bit image written from it: round half to even, saturate"""
    img = image_u8.astype(np.float32) / np.float32(255.0)
    R = R.astype(np.float32)
    t = ((img + R) - img * R) * np.float32(255.0)
    return np.clip(np.rint(t), 0, 255).astype(np.uint8)


def synthesize_host(image_u8, mask_u8, plan, warp=warp_pillow):
    """image_u8, mask_u8: uint8 [H,W,3] RGB numpy arrays of one size -> the rainy image, uint8 [H,W,3]"""
    assert image_u8.shape == mask_u8.shape and image_u8.dtype == mask_u8.dtype == np.uint8 and image_u8.shape[2] == 3
    return composite_host(image_u8, mix_host(mask_u8, plan, warp))


# ---------------------------------------------------------------------------------------------------- device
def scratch_bytes(H, W, depth):
    from .. import _lib

    n = ctypes.c_size_t(0)
    _lib.call("dadet_rain_scratch_bytes", int(H), int(W), int(depth), ctypes.byref(n))
    return int(n.value)


def synthesize_device(image_u8, mask_u8, plan, out=None, scratch=None):
    """the same on the HIP device, on the current stream: image_u8 / mask_u8 uint8 [H,W,3] device tensors -> uint8 [H,W,3].
    At most three launches for the reference's depths (2 or 3).  `scratch`: a uint8 device tensor to reuse (at least
    scratch_bytes(H, W, plan.depth) elements); allocated when missing or too small."""
    import torch

    from .. import _lib

    if not (image_u8.is_cuda and mask_u8.is_cuda):
        raise _lib.DadetError("synthesize_device: image and mask must live on the HIP device")
    assert image_u8.dtype == mask_u8.dtype == torch.uint8 and image_u8.dim() == 3 and image_u8.shape[2] == 3
    assert tuple(image_u8.shape) == tuple(mask_u8.shape), "the mask must already have the image's size"
    image_u8, mask_u8 = image_u8.contiguous(), mask_u8.contiguous()
    H, W = int(image_u8.shape[0]), int(image_u8.shape[1])
    dev = image_u8.device
    need = scratch_bytes(H, W, plan.depth)
    if scratch is None or scratch.numel() < need:
        scratch = torch.empty(max(need, 4), dtype=torch.uint8, device=dev)
    assert scratch.dtype == torch.uint8 and scratch.device == dev and scratch.is_contiguous()
    if out is None:
        out = torch.empty_like(image_u8)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (H, W, 3) and out.is_contiguous() and out.device == dev
    coeffs = np.ascontiguousarray(plan.coeffs, dtype=np.float64)
    assert coeffs.shape == (WIDTH, plan.depth, 6)
    ws = (ctypes.c_float * 3)(*[float(v) for v in plan.ws])
    stream = torch.cuda.current_stream(dev)
    _lib.call("dadet_rain_synthesize", ctypes.c_void_p(image_u8.data_ptr()), ctypes.c_void_p(mask_u8.data_ptr()), H, W,
              int(plan.depth), coeffs.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ws, float(plan.c0), float(plan.c1),
              ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(scratch.data_ptr()), int(scratch.numel()),
              ctypes.c_void_p(stream.cuda_stream))
    for t in (image_u8, mask_u8, scratch, out):       # (they may have been allocated on another stream)
        t.record_stream(stream)
    return out


def upload(array_u8, device):
    """a numpy image -> device tensor through a pinned copy, like the loader's staging buffers (no transfer of this size
    straight from pageable memory)"""
    import torch

    return torch.from_numpy(np.ascontiguousarray(array_u8)).pin_memory().to(device)


# ----------------------------------------------------------------------------------------------------- masks
class RainMasks(object):
    """the rain-mask images of a folder, sorted by file name.  `host_mask(i, (W, H))` is mask i as uint8 [H,W,3] RGB at
    that size (Pillow convert("RGB"), Image.resize(BILINEAR)), `device_mask` the same as a device tensor; both cached
    per (mask, size), the caches bounded (a Cityscapes-size mask is 6 MB) and left behind when the object is pickled."""

    EXTENSIONS = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff")

    def __init__(self, directory, host_cache=16, device_cache=16):
        self.directory = directory
        self.files = sorted(f for f in os.listdir(directory) if f.lower().endswith(self.EXTENSIONS))
        if not self.files:
            raise ValueError("no rain-mask image in %s" % directory)
        self._limits = (host_cache, device_cache)
        self._host, self._device = collections.OrderedDict(), collections.OrderedDict()

    def __len__(self):
        return len(self.files)

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_host"], state["_device"] = collections.OrderedDict(), collections.OrderedDict()
        return state

    @staticmethod
    def _cached(cache, key, limit, make):
        if key in cache:
            cache.move_to_end(key)
            return cache[key]
        value = make()
        cache[key] = value
        while len(cache) > limit:
            cache.popitem(last=False)
        return value

    def _read(self, index, size):
        from PIL import Image

        img = Image.open(os.path.join(self.directory, self.files[index])).convert("RGB")
        if img.size != tuple(size):
            img = img.resize(tuple(size), Image.BILINEAR)
        return np.array(img, dtype=np.uint8)

    def host_mask(self, index, size):
        size = (int(size[0]), int(size[1]))
        return self._cached(self._host, (index, size), self._limits[0], lambda: self._read(index, size))

    def device_mask(self, index, size, device):
        size = (int(size[0]), int(size[1]))
        return self._cached(self._device, (index, size, str(device)), self._limits[1],
                            lambda: upload(self.host_mask(index, size), device))
