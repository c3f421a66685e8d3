"""A stand-in detector for the test-time augmentation tests: the same class runs under the reference's
`im_detect_bbox_aug` (tests/golden/make_golden_bbox_aug.py) and under this package's (tests/test_bbox_aug.py) — the BoxList
constructor is injected, nothing else of either package is touched.

Per call (one augmentation pass) it LOGS what it was given — per image the size, the sum over the valid region, four probe
pixels and whether the left half is brighter than the right — and RETURNS the unfiltered form a post-processor with
bbox_aug_enabled hands out: boxes [R * C, 4] and scores [R * C].  The boxes are an exact function of the pass's image size
and a seeded table: fractions of the size, rounded down to multiples of 1/4 on the host in float64, so they are the same
float32 numbers wherever the pass runs.  The scores come from the same seeded stream, one table per pass (eight of them,
then they repeat), so that the passes differ and no two candidates of a merged list share a score: the reference's CPU NMS
ranks with an unstable sort, and the order of exactly tied scores is not defined there."""
import numpy as np
import torch

PROBES = ((0.25, 0.25), (0.25, 0.75), (0.5, 0.5), (0.8, 0.1))      # (row, column) as fractions of the valid size


def make_images(seed=7):
    """two small uint8 RGB images of different sizes, each with a bright left half (so a mirrored pass shows)"""
    rng = np.random.default_rng(seed)
    out = []
    for h, w in ((60, 100), (72, 90)):
        im = rng.integers(0, 120, (h, w, 3), dtype=np.uint8)
        im[:, : w // 2] += 100
        out.append(im)
    return out


class StubDetector(object):
    def __init__(self, make_boxlist, num_classes=4, rows=24, seed=11, empty=False):
        self.make_boxlist = make_boxlist          # (boxes float32 [n, 4] tensor, (w, h)) -> BoxList in xyxy mode
        self.num_classes, self.rows, self.empty = num_classes, rows, empty
        rng = np.random.default_rng(seed)
        k = max(1, rows // 4)                     # rows / 4 clusters: NMS has something to remove
        centre = rng.uniform(0.2, 0.8, (k, 2))
        side = rng.uniform(0.1, 0.35, (k, 2))
        which = rng.integers(0, k, rows)
        jitter = rng.uniform(-0.02, 0.02, (rows, num_classes, 4))
        c, s = centre[which][:, None, :], side[which][:, None, :]
        self.frac = np.clip(np.concatenate([c - s / 2, c + s / 2], -1) + jitter, 0.0, 1.0)      # [R, C, 4] in [0, 1]
        logits = rng.normal(0, 1.5, (8, rows, num_classes))
        e = np.exp(logits - logits.max(2, keepdims=True))
        self.scores = (e / e.sum(2, keepdims=True)).astype(np.float32)          # [pass % 8, R, C]
        self.calls = []

    def eval(self):
        return self

    def boxes_for(self, w, h):
        scale = np.array([w - 1, h - 1, w - 1, h - 1], np.float64)
        return (np.floor(self.frac * scale * 4.0) / 4.0).astype(np.float32).reshape(-1, 4)

    def __call__(self, image_list, targets=None):
        tensors = image_list.tensors.detach().cpu().double()
        record = {"padded": tuple(tensors.shape[-2:]), "sizes": [], "sums": [], "probes": [], "left_brighter": []}
        out = []
        for i, (h, w) in enumerate(image_list.image_sizes):
            h, w = int(h), int(w)
            t = tensors[i, :, :h, :w]
            record["sizes"].append((w, h))
            record["sums"].append(float(t.sum()))
            record["probes"].append([float(t[c % 3, int(fy * h), int(fx * w)]) for c, (fy, fx) in enumerate(PROBES)])
            record["left_brighter"].append(bool(t[:, :, : w // 2].mean() > t[:, :, w - w // 2:].mean()))
            device = image_list.tensors.device
            if self.empty:
                boxes, scores = torch.zeros((0, 4)), torch.zeros((0,))
            else:
                boxes = torch.from_numpy(self.boxes_for(w, h))
                scores = torch.from_numpy(self.scores[len(self.calls) % 8].reshape(-1).copy())
            boxlist = self.make_boxlist(boxes.to(device), (w, h))
            boxlist.add_field("scores", scores.to(device))
            out.append(boxlist)
        self.calls.append(record)
        return out
