"""The error bars of the direct float64 parity tests (tests/test_da_heads_gpu.py derives them; test_losses_gpu.py and
test_elementwise_gpu.py use the same ones).  u = 2^-24.
  a value that is one chain of multiplications / divisions:  16 u |ref| + one fp32 denormal step;
  a sum of n values of k leaves each:  (n + k + 1 + 16) u S,  S = sum of the reference's leaf magnitudes.
Every check prints its largest err / bound ratio."""
import numpy as np
import torch

U = 2.0 ** -24
FLOOR = 2.0 ** -149                      # one fp32 denormal step


def f32(v):
    return float(np.float32(v))


def check(name, got, ref, bound):
    got = got.detach().to("cpu", torch.float64)
    ref = ref.detach().to(torch.float64)
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), name + ": non-finite"
    bound = torch.as_tensor(bound, dtype=torch.float64).broadcast_to(ref.shape)
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)       # a zero bound admits only the exact value
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print("    %-34s max err / bound = %.4f   (n = %d)" % (name, worst, ratio.numel()))
    assert worst <= 1.0, "%s: err / bound = %.3f" % (name, worst)
    return worst


def elem_bound(ref):
    return 16 * U * ref.abs() + FLOOR


def sum_bound(n, abs_sum, leaves=1):
    return (n + leaves + 1 + 16) * U * abs_sum


def spread(shape, g):
    """magnitudes over about six decades: another order of summation rounds differently"""
    return torch.randn(shape, generator=g) * 10.0 ** (torch.rand(shape, generator=g) * 6 - 3)
