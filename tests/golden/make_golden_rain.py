"""Golden record for the rain layer — runs ONLY in the authoring container (needs /root/reference).

Imports the reference's efficientderain-master/augment_and_mix.py (and the augmentations.py it imports) by path and
stores DATA ONLY in tests/golden/rain_mix.npz: per case the seed, a uint8 mask [H,W,3] and the float32 array
`augment_and_mix(float32(mask) / 255, severity=3, width=3, depth=-1)` returns under `np.random.seed(seed)`.

The masks are streaky — a power of uniform noise smeared along a slant, most pixels near 0 and a few near 255 — so that
warped zeros and sums above 1 both occur.  The seeds were chosen so that both depths (2 and 3) and all seven operators
occur and at least one case exceeds 1; tests/test_rain_host.py asserts that on the plans it draws itself.

    python tests/golden/make_golden_rain.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/efficientderain-master"
CASES = [(3, 19, 23), (1, 33, 65), (21, 40, 72), (23, 19, 23), (25, 33, 65), (4, 40, 72)]      # (seed, H, W)


def streaky_mask(seed, H, W):
    rng = np.random.default_rng(1000 + seed)
    noise = rng.random((H + 8, W + 8)) ** 6
    streak = sum(np.roll(np.roll(noise, k, axis=0), k // 2, axis=1) for k in range(6))[4:H + 4, 4:W + 4]
    grey = np.clip(streak * 260.0 - 8.0, 0, 255)
    return np.stack([grey, grey * 0.97, np.clip(grey * 1.05, 0, 255)], axis=2).astype(np.uint8)


def main():
    sys.path.insert(0, REF)
    import augment_and_mix

    out = {"seeds": np.array([c[0] for c in CASES], dtype=np.int64)}
    for seed, H, W in CASES:
        mask = streaky_mask(seed, H, W)
        layer = mask.astype(np.float32) / 255.0
        np.random.seed(seed)
        mixed = augment_and_mix.augment_and_mix(layer, severity=3, width=3, depth=-1)
        assert mixed.dtype == np.float32 and mixed.shape == mask.shape
        out["mask_%d" % seed] = mask
        out["mixed_%d" % seed] = mixed
        print(seed, (H, W), "max %.3f" % mixed.max(), "zeros %.2f" % (mask == 0).mean())
    path = os.path.join(HERE, "rain_mix.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
