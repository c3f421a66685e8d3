"""Outputs of the REFERENCE's own compiled CPU operators (oracle/_ref/ref_C.so, built by oracle/build_ref.py) on the inputs
of two tests, stored in tests/golden/ref_build_outputs.npz so that neither test needs the reference build at run time:
  * cpu/*: tests/test_oracle_golden.py::test_ops_match_live_reference_build (the CPU oracle), inputs stored in full;
  * gpu/*: tests/test_ops_gpu.py::test_hip_ops_against_the_reference_build_itself (the HIP operators).  Its largest ROIAlign
    input is 4 MB, so the inputs are regenerated from a seed by `gpu_cases()` below and only SHA-256 digests of the
    inputs (to prove the regenerated inputs are the ones the reference saw) and of the ROIAlign outputs are stored; NMS
    kept indices are stored in full.
Authoring container only (needs the reference build); `gpu_cases()` and `sha256()` are imported by the GPU test."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "ref_build_outputs.npz")
NMS_SIZES = (1, 37, 2000, 12000)
# C, H, W, R, pooled size, sampling ratio
ROI_SHAPES = [(32, 24, 40, 50, 7, 2), (64, 64, 128, 128, 14, 0), (8, 13, 21, 20, 14, 0)]


def sha256(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def gpu_cases():
    """-> (nms: [(n, boxes, scores)], roi: [((C, H, W, R, ph, sr), x, rois)]), float32, from numpy's PCG64 stream"""
    rng = np.random.default_rng(21)
    nms = []
    for n in NMS_SIZES:
        xy = rng.random((n, 2)) * np.array([1900.0, 950.0])
        boxes = np.concatenate([xy, xy + rng.random((n, 2)) * 250 + 2], 1).astype(np.float32)
        scores = rng.random(n).astype(np.float32)
        nms.append((n, boxes, scores))
    roi = []
    for shape in ROI_SHAPES:
        C, H, W, R, ph, sr = shape
        x = rng.standard_normal((2, C, H, W)).astype(np.float32)
        xy = rng.random((R, 2)) * np.array([W * 14.0, H * 14.0])
        batch = rng.integers(0, 2, (R, 1))
        wh = rng.random((R, 2)) ** 2 * 400 + 1
        rois = np.concatenate([batch, xy, xy + wh], 1).astype(np.float32)
        roi.append((shape, x, rois))
    return nms, roi


def main():
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from oracle import build_ref

    build_ref.build()
    ref = build_ref.load()
    assert ref is not None, "the reference build is needed to write this fixture"
    t = torch.from_numpy
    out = {}
    rng = np.random.default_rng(7)
    x = rng.standard_normal((2, 6, 17, 23)).astype(np.float32)
    rois = np.concatenate([rng.integers(0, 2, (30, 1)), rng.uniform(-10, 200, (30, 2)),
                           rng.uniform(150, 420, (30, 2))], 1).astype(np.float32)
    boxes = np.concatenate([rng.uniform(0, 300, (800, 2)), rng.uniform(300, 500, (800, 2))], 1).astype(np.float32)
    scores = (rng.permutation(800) / 800.0).astype(np.float32)
    out.update({"cpu/x": x, "cpu/rois": rois, "cpu/boxes": boxes, "cpu/scores": scores,
                "cpu/roi_out": ref.roi_align_forward(t(x), t(rois), 1 / 16.0, 7, 7, 0).numpy(),
                "cpu/keep": ref.nms(t(boxes), t(scores), 0.6).numpy()})
    nms, roi = gpu_cases()
    for n, boxes, scores in nms:
        out["gpu/nms_inputs_sha256_%d" % n] = np.array(sha256(boxes, scores))
        out["gpu/nms_keep_%d" % n] = ref.nms(t(boxes), t(scores), 0.7).numpy()
    for i, ((C, H, W, R, ph, sr), x, rois) in enumerate(roi):
        out["gpu/roi_inputs_sha256_%d" % i] = np.array(sha256(x, rois))
        want = ref.roi_align_forward(t(x), t(rois), 1 / 16.0, ph, ph, sr).numpy()
        out["gpu/roi_out_sha256_%d" % i] = np.array(sha256(want))
    np.savez_compressed(PATH, **out)
    print("wrote", PATH, os.path.getsize(PATH) // 1024, "KB")


if __name__ == "__main__":
    main()
