"""dadet_nms_batch: NMS of a batch of pre-ranked images in one launch per stage.  Kept positions and counts must be EXACTLY
those of the single-image call `_C.nms_with_count(boxes_i, None, ...)` for every image: the batched kernels run the
single-image kernels' device bodies on the same arguments, so anything else is an indexing error between images."""
import ctypes

import numpy as np
import pytest
import torch

from test_ops_gpu import _rand_boxes

pytestmark = pytest.mark.gpu
N_CHOICES = (0, 1, 63, 64, 65, 255, 256, 257, 1000)


def _ranked_boxes(seed, n, max_side=150):
    """the seeded maker of test_nms_three_sweeps_agree_with_the_oracle; the rows ARE the ranking (best first)"""
    rng = np.random.default_rng(seed)
    return _rand_boxes(rng, max(n, 1), max_side=max_side)[:n]


def _chain(n):
    """every box overlaps the first one above the threshold: one kept box, everything else suppressed through block after
    block of the sweep"""
    b = np.zeros((n, 4), np.float32)
    b[:, 0] = np.arange(n) % 7 * 0.25
    b[:, 1] = np.arange(n) % 5 * 0.25
    b[:, 2] = b[:, 0] + 400
    b[:, 3] = b[:, 1] + 300
    return b


def _apart(n):
    """no two boxes touch: everything is kept"""
    i = np.arange(n)
    x, y = (i % 40) * 50.0, (i // 40) * 50.0
    return np.stack([x, y, x + 30, y + 30], 1).astype(np.float32)


def _batch(images, device):
    n_max = max(max(len(b) for b in images), 1)
    boxes = torch.full((len(images), n_max, 4), float("nan"))        # what lies behind an image's count must not matter
    for i, b in enumerate(images):
        boxes[i, : len(b)] = torch.from_numpy(b)
    return boxes.to(device), [len(b) for b in images]


def _check(boxes, counts, thresh, max_keep, tie_rule):
    from da_detect_amd import _C

    keep, num = _C.nms_batch_with_count(boxes, counts, thresh, max_keep=max_keep, tie_rule=tie_rule)
    assert tuple(keep.shape) == tuple(boxes.shape[:2]) and tuple(num.shape) == (len(counts),)
    num = num.tolist()
    kept = []
    for i, n in enumerate(counts):
        if n == 0:
            assert num[i] == 0
            kept.append([])
            continue
        k1, c1 = _C.nms_with_count(boxes[i, :n].contiguous(), None, thresh, max_keep=max_keep, tie_rule=tie_rule)
        want = k1[: int(c1)].tolist()
        assert num[i] == len(want), "image %d (n = %d): %d kept, single-image call %d" % (i, n, num[i], len(want))
        assert keep[i, : num[i]].tolist() == want, "image %d (n = %d): kept positions differ" % (i, n)
        kept.append(want)
    return kept


BATCHES = {
    1: [[n] for n in N_CHOICES],
    2: [[N_CHOICES[i], N_CHOICES[(i + 4) % 9]] for i in range(9)],
    # the largest image first, in the middle and last; an empty image first, inside and last
    5: [[1000, 0, 63, 256, 65], [1, 255, 1000, 64, 257], [0, 257, 1, 65, 1000], [64, 63, 255, 256, 0]],
}


def test_nms_batch_cases_cover_every_count():
    for lists in BATCHES.values():
        assert {n for ns in lists for n in ns} == set(N_CHOICES)


@pytest.mark.parametrize("tie_rule", [0, 1])
@pytest.mark.parametrize("batch", [1, 2, 5])
def test_nms_batch_equals_per_image_calls(device, batch, tie_rule):
    """every per-image count of N_CHOICES at every batch size, mixed within one batch, with and without a quota"""
    for case, ns in enumerate(BATCHES[batch]):
        assert len(ns) == batch
        images = [_ranked_boxes(100 * case + 7 * i + tie_rule, n, max_side=(400 if i % 2 else 150))
                  for i, n in enumerate(ns)]
        boxes, counts = _batch(images, device)
        for max_keep in (-1, 40):
            _check(boxes, counts, 0.7, max_keep, tie_rule)


@pytest.mark.parametrize("tie_rule", [0, 1])
def test_nms_batch_chain_apart_and_quota(device, tie_rule):
    """one image whose boxes all overlap (a long suppression chain, one kept box) beside one without overlaps (everything
    kept); a quota reached in the middle of a 256-box block for one image (the spread-out one: position 300 of 1000) and
    never for its neighbours"""
    images = [_chain(1000), _apart(1000), _ranked_boxes(3, 257, max_side=400), _chain(65)]
    boxes, counts = _batch(images, device)
    kept = _check(boxes, counts, 0.7, -1, tie_rule)
    assert kept[0] == [0] and kept[1] == list(range(1000)) and kept[3] == [0]
    kept = _check(boxes, counts, 0.7, 300, tie_rule)
    assert kept[0] == [0] and kept[1] == list(range(300)) and 1 < len(kept[2]) < 300


def test_nms_batch_all_empty_and_short_workspace(device):
    from da_detect_amd import _C, _lib

    boxes = torch.zeros((3, 8, 4), device=device)
    keep, num = _C.nms_batch_with_count(boxes, [0, 0, 0], 0.7)
    assert num.tolist() == [0, 0, 0]
    images = [_ranked_boxes(1, 300), _ranked_boxes(2, 64)]
    boxes, counts = _batch(images, device)
    nbytes = ctypes.c_size_t(0)
    _lib.call("dadet_nms_batch_workspace_bytes", 2, 300, ctypes.byref(nbytes))
    one = ctypes.c_size_t(0)
    _lib.call("dadet_nms_workspace_bytes", 300, ctypes.byref(one))
    assert nbytes.value == 2 * one.value
    exact = torch.empty(nbytes.value, dtype=torch.uint8, device=device)
    _C.nms_batch_with_count(boxes, counts, 0.7, workspace=exact)
    short = torch.empty(nbytes.value - 1, dtype=torch.uint8, device=device)
    with pytest.raises(_lib.DadetError, match="workspace"):
        _C.nms_batch_with_count(boxes, counts, 0.7, workspace=short)
    with pytest.raises(_lib.DadetError):
        _C.nms_batch_with_count(boxes, [301, 64], 0.7)                  # a count beyond n_max
    with pytest.raises(_lib.DadetError):
        _C.nms_batch_with_count(torch.zeros((65, 4, 4), device=device), [4] * 65, 0.7)      # more than 64 images
