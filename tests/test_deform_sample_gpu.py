"""The deformable sampling kernels of csrc/deform.hip called directly (_C.deform_sample_forward / _backward and their
`_om` forms, no GEMM on top) against oracle/deform_ref.deform_sample in float64, every backward form by name.

Inputs.  Offsets are multiples of 1/16 chosen so that every sampling position has a fractional part in [2/16, 14/16] in
both axes: the float32 position (ho * s - pad + i * dil) + off equals the float64 one exactly, no floor can flip, no
one-sided derivative is involved and nothing is masked out of a comparison (the one exception is
test_exact_positions, which says what it leaves out).

Tolerance.  For every compared quantity e_k = max|kernel - ref64| / max|ref64| and e_32 = the same figure of the same
oracle evaluated in float32 on the CPU; required: e_k <= 4 * e_32 + 2^-22.  The factor 4 is for the different summation
order (atomics, wave reductions, lists), the floor for quantities the float32 oracle happens to get exactly.  Both
figures are printed per case and quantity (lines starting with "DSAMPLE").

Which form runs is asserted per case through dadet_deform_sample_backward_form, the launcher's own choice:
0 the plain atomic kernel, 1 the LDS-window kernel, 2 the two-pass gather.  The gather cases also state the longest
per-position list (kListCap = 32 entries, further samples overflow into float atomics), counted on the CPU by
longest_list, a mirror of tl_list.

Largest observed e_k / e_32 per form on an MI355X (over all quantities; the bound allows 4 plus the floor; the figures of
the atomic forms move a little from run to run with the order in which the adds arrive):
  forward      1.00  every case: cols has the float32 oracle's own error (the same operation order)
  plain        3.00  x_plain gx (e_k 2.62e-07, 0.45 of its bound); without the exact-position case 1.91 (p_c8_k13 gx)
  LDS window   1.75  x_lds gx (1.66e-07, 0.27 of its bound); without the exact-position case 1.54 (om_lds_nows gx)
  gather       2.13  g_over_e_two gx (3.66e-07, 0.40 of its bound); lists only: 1.69 (x_gather gx)
  the overflow cases, gx: (a) 0.82, (b) 1.00, (c) 0.75 (2.62e-07 against 3.50e-07), (d) 0.99, (e) 2.13
  `_om` form against the dense form on the sliced tensors: at most 1.36e-07 of the maximum (gx), 2.7e-08 (gom)
Pass A sums the overflowed samples of a wavefront that share a position before one of them sends the sum by float atomics.
With one atomic per overflowed sample, case (c) — 1048 of 1080 samples a serial float32 chain on four addresses — was off
by 1.714e-06 (ratio 4.90: over the bound) and (d) by 7.05e-07 (ratio 4.00); a float32 sum of the same terms taken one by
one is off by 0.7e-06 .. 1.5e-06 on the CPU, the oracle's blocked sum by 3.5e-07: summation order.
"""
import ctypes
import functools
import zlib
from collections import namedtuple

import numpy as np
import pytest
import torch

CL = torch.channels_last
PLAIN, LDS, GATHER = 0, 1, 2
FORM_NAME = {None: "forward", PLAIN: "plain", LDS: "lds", GATHER: "gather"}
TOL_FACTOR, TOL_FLOOR = 4.0, 2.0 ** -22

# rng: integer parts of the offsets are drawn from [-rng, rng); aim: None, or one top-left position (hl, wl) per deformable
# group on which EVERY sample of the group lands (the overflow cases; a pair of positions: see make_offsets); longest: what
# longest_list must answer
Case = namedtuple("Case", "name N C H W kh kw stride pad dil dg modulated rng aim workspace need_x form longest")


def _c(name, N, C, H, W, k, stride, pad, dil, dg, modulated, rng=2, aim=None, workspace=True, need_x=True, form=None,
       longest=None):
    kh, kw = (k, k) if isinstance(k, int) else k
    return Case(name, N, C, H, W, kh, kw, stride, pad, dil, dg, modulated, rng, aim, workspace, need_x, form, longest)


def out_size(c):
    return ((c.H + 2 * c.pad - (c.dil * (c.kh - 1) + 1)) // c.stride + 1,
            (c.W + 2 * c.pad - (c.dil * (c.kw - 1) + 1)) // c.stride + 1)


FORWARD_CASES = [
    # C = 8: 128 pixels per workgroup; N * Ho * Wo = 63 and 129 leave the last workgroup ragged
    _c("f_c8_63px", 1, 8, 7, 9, 1, 1, 0, 1, 1, False),
    _c("f_c8_63px_dg2", 1, 8, 7, 9, 1, 1, 0, 1, 2, True),
    _c("f_c8_129px", 1, 8, 3, 43, 1, 1, 0, 1, 2, True),
    _c("f_c8_129px_k3", 1, 8, 3, 43, 3, 1, 1, 1, 1, False),
    _c("f_c12", 2, 12, 7, 9, 3, 1, 1, 1, 1, True),                 # 3 lanes: does not divide 256
    _c("f_c192_dg4", 1, 192, 7, 9, 3, 1, 1, 1, 4, True),
    _c("f_c192_k13", 2, 192, 3, 43, (1, 3), 1, 1, 1, 2, False),
    _c("f_c1024_dg4", 1, 1024, 7, 9, 3, 1, 1, 1, 4, True),        # lanes == blockDim
    _c("f_c1280", 1, 1280, 7, 9, (3, 1), 1, 1, 1, 1, True),        # channel loop with a tail
    _c("f_c1280_dg4_s2", 1, 1280, 7, 9, 3, 2, 1, 1, 4, False),
    _c("f_c192_s2", 2, 192, 7, 9, 3, 2, 1, 1, 1, True),
    _c("f_c64_dil2", 1, 64, 7, 9, 3, 1, 2, 2, 2, True),
    _c("f_c8_dil2_k31", 1, 8, 7, 9, (3, 1), 1, 2, 2, 1, False),
]

PLAIN_CASES = [
    _c("p_c8_dg2", 2, 8, 7, 9, 3, 1, 1, 1, 2, True, form=PLAIN),             # 4 channels per group: per-lane atomics
    _c("p_c512_dg4", 1, 512, 7, 9, 3, 2, 1, 1, 4, True, form=PLAIN),         # 128 per group: not wave-uniform
    _c("p_c1024_dg4", 1, 1024, 7, 9, 3, 1, 2, 2, 4, True, form=PLAIN),       # 256 per group: wave-uniform with dg > 1
    _c("p_c1280", 1, 1280, 7, 9, 3, 2, 1, 1, 1, False, form=PLAIN),          # second trip of the channel loop, 3 idle waves
    _c("p_c64_s2", 2, 64, 7, 9, 3, 2, 1, 1, 1, True, form=PLAIN),
    _c("p_c64_dil2", 1, 64, 7, 9, 3, 1, 2, 2, 1, True, form=PLAIN),          # stride 1, C % 64 == 0, and still plain
    _c("p_c8_k13", 1, 8, 3, 43, (1, 3), 1, 1, 1, 1, False, form=PLAIN),
]

LDS_CASES = [
    # no workspace (the C consumer's dadet_deform_sample_backward): 64-channel chunks inside one group, one wave reduction
    _c("l_nows_c64", 1, 64, 9, 17, 3, 1, 1, 1, 1, True, rng=2, workspace=False, form=LDS),       # |offset| < 2.5: in window
    _c("l_nows_c128_dg2", 2, 128, 20, 19, 3, 1, 1, 1, 2, False, rng=6, workspace=False, form=LDS),  # +-6: global atomics too
    _c("l_nows_c64_k31", 1, 64, 9, 17, (3, 1), 1, 1, 1, 1, True, rng=6, workspace=False, form=LDS),
    # with the workspace: 16 / 32 channels per group keep the gather out
    _c("l_c64_dg4_k1", 2, 64, 9, 17, 1, 1, 0, 1, 4, True, rng=6, form=LDS),
    _c("l_c64_dg2", 1, 64, 20, 19, 3, 1, 1, 1, 2, False, rng=2, form=LDS),
    _c("l_c128_dg8", 1, 128, 9, 17, 3, 1, 1, 1, 8, True, rng=6, form=LDS),
]

GATHER_CASES = [
    _c("g_c64_wo5", 2, 64, 6, 5, 3, 1, 1, 1, 1, True, form=GATHER, longest=("le", 32)),
    _c("g_c128_dg2_wo7_k1", 1, 128, 5, 7, 1, 1, 0, 1, 2, False, form=GATHER, longest=("le", 32)),
    _c("g_c64_wo8_k13", 2, 64, 3, 8, (1, 3), 1, 1, 1, 1, True, form=GATHER, longest=("le", 32)),   # a step with off taps
    _c("g_c64_w5_wo7_k31", 1, 64, 6, 5, (3, 1), 1, 1, 1, 1, False, form=GATHER, longest=("le", 32)),
    _c("g_c128_dg2_wo7", 1, 128, 6, 7, 3, 1, 1, 1, 2, True, form=GATHER, longest=("le", 32)),
    _c("g_c128_dg2_no_gx", 2, 128, 6, 7, 3, 1, 1, 1, 2, True, need_x=False, form=GATHER, longest=("le", 32)),
    # (a) all 32 pixels on one interior position: the list is exactly full, nothing overflows
    _c("g_over_a_32", 1, 64, 4, 8, 1, 1, 0, 1, 1, True, aim=((1, 3),), form=GATHER, longest=("eq", 32)),
    # (b) 33 samples: one overflow (per group)
    _c("g_over_b_33", 1, 128, 3, 11, 1, 1, 0, 1, 2, False, aim=((1, 5), (0, 8)), form=GATHER, longest=("eq", 33)),
    # (c) every sample of every pixel on one interior position, all four corners live
    _c("g_over_c_1080", 1, 64, 10, 12, 3, 1, 1, 1, 1, True, aim=((4, 6),), form=GATHER, longest=("ge", 1000)),
    # (e) two positions, alternating by pixel and with the middle tap of each step swapped: the wavefront's pre-sum of
    # overflowed samples merges pixels 0 / 2 and 1 / 3 but not neighbours, and taps 0 / 2 but not tap 1
    _c("g_over_e_two", 1, 64, 10, 12, 3, 1, 1, 1, 1, True, aim=(((4, 6), (2, 3)),), form=GATHER, longest=("eq", 540)),
    # (d) the same in the band h in (-1, 0): two corners live
    _c("g_over_d_band", 1, 64, 10, 12, 3, 1, 1, 1, 1, True, aim=((-1, 5),), form=GATHER, longest=("ge", 33)),
]

BACKWARD_CASES = PLAIN_CASES + LDS_CASES + GATHER_CASES

# the `_om` forms, once per backward form (the LDS window with and without the workspace); ld = the channels used, padded
OM_CASES = [
    _c("om_plain_dg2", 1, 8, 7, 9, 3, 1, 1, 1, 2, True, form=PLAIN),                        # 54 -> 56
    _c("om_lds_nows", 1, 64, 9, 17, 3, 1, 1, 1, 1, False, workspace=False, form=LDS),         # 18 -> 20
    _c("om_lds_dg2", 1, 64, 9, 11, 3, 1, 1, 1, 2, True, form=LDS),                           # 54 -> 56
    _c("om_gather", 2, 64, 6, 7, 3, 1, 1, 1, 1, True, form=GATHER, longest=("le", 32)),      # 27 -> 28
]

EXACT_CASES = [
    _c("x_plain", 1, 8, 7, 9, 3, 1, 1, 1, 2, True, form=PLAIN),
    _c("x_lds", 1, 64, 7, 9, 3, 1, 1, 1, 4, True, form=LDS),
    _c("x_gather", 1, 64, 7, 9, 3, 1, 1, 1, 1, True, form=GATHER, longest=("le", 32)),
]

_ids = lambda cases: [c.name for c in cases]


# ---------------------------------------------------------------------------------------------------------------
# inputs
def _gen(c, salt=0):
    return torch.Generator().manual_seed(zlib.crc32(c.name.encode()) + salt)


def _base(c):
    Ho, Wo = out_size(c)
    ys = (torch.arange(Ho, dtype=torch.float64) * c.stride - c.pad).view(Ho, 1)
    xs = (torch.arange(Wo, dtype=torch.float64) * c.stride - c.pad).view(1, Wo)
    return ys, xs


def make_offsets(c, g):
    """[N, dg*2*T, Ho, Wo] float32, multiples of 1/16, fractional parts of every position in [2/16, 14/16]"""
    Ho, Wo = out_size(c)
    T = c.kh * c.kw
    shape = (c.N, c.dg, T, 2, Ho, Wo)
    frac = torch.randint(2, 15, shape, generator=g).double() / 16
    if c.aim is None:
        off = torch.randint(-c.rng, c.rng, shape, generator=g).double() + frac
    else:
        ys, xs = _base(c)
        off = torch.empty(shape, dtype=torch.float64)
        for grp in range(c.dg):
            for tap in range(T):
                i, j = tap // c.kw, tap % c.kw
                a = c.aim[grp]
                if isinstance(a[0], tuple):      # two positions: odd pixels and the middle tap of a step swap them
                    pick = ((torch.arange(Wo).view(1, Wo) + (1 if tap % 3 == 1 else 0)) % 2).double()
                    ah, aw = a[0][0] + (a[1][0] - a[0][0]) * pick, a[0][1] + (a[1][1] - a[0][1]) * pick
                else:
                    ah, aw = a
                off[:, grp, tap, 0] = ah + frac[:, grp, tap, 0] - (ys + i * c.dil)
                off[:, grp, tap, 1] = aw + frac[:, grp, tap, 1] - (xs + j * c.dil)
    off = off.reshape(c.N, c.dg * 2 * T, Ho, Wo)
    assert torch.equal(off.float().double(), off)
    return off.float()


@functools.lru_cache(maxsize=None)
def make_inputs(c):
    """x, offset, mask | None, gcols (logical NCHW, float32, on the CPU); gcols channel = tap * C + c"""
    g = _gen(c)
    Ho, Wo = out_size(c)
    T = c.kh * c.kw
    x = torch.randn((c.N, c.C, c.H, c.W), generator=g)
    off = make_offsets(c, g)
    mask = torch.rand((c.N, c.dg * T, Ho, Wo), generator=g) if c.modulated else None
    gcols = torch.randn((c.N, T * c.C, Ho, Wo), generator=g)
    return x, off, mask, gcols


def longest_list(c, off):
    """the longest per-position sample list of the gather form for these offsets.  Mirror of tl_list (csrc/deform.hip): one
    list per (image, top-left position (hl, wl) in [-1, H-1] x [-1, W-1], deformable group), one entry per VALID sample
    (pixel, tap) whose bilinear footprint starts there"""
    T = c.kh * c.kw
    ys, xs = _base(c)
    counts = np.zeros((c.N, c.H + 1, c.W + 1, c.dg), dtype=np.int64)
    off = off.double()
    n_idx = np.arange(c.N).reshape(c.N, 1, 1) + np.zeros(off.shape[2:], dtype=np.int64)
    for grp in range(c.dg):
        for tap in range(T):
            i, j = tap // c.kw, tap % c.kw
            h = (ys + i * c.dil + off[:, grp * 2 * T + 2 * tap]).numpy()
            w = (xs + j * c.dil + off[:, grp * 2 * T + 2 * tap + 1]).numpy()
            valid = (h > -1) & (w > -1) & (h < c.H) & (w < c.W)
            hl, wl = np.floor(h).astype(np.int64), np.floor(w).astype(np.int64)
            np.add.at(counts, (n_idx[valid], hl[valid] + 1, wl[valid] + 1, grp), 1)
    return int(counts.max())


# ---------------------------------------------------------------------------------------------------------------
# the oracle in float64 and float32
def _oracle(c, x, off, mask, gcols, dtype):
    from oracle import deform_ref as R

    Ho, Wo = out_size(c)
    T = c.kh * c.kw
    leaves = [t.to(dtype).clone().requires_grad_(True) if t is not None else None for t in (x, off, mask)]
    cols = R.deform_sample(leaves[0], leaves[1], leaves[2], c.kh, c.kw, c.stride, c.pad, c.dil, c.dg)   # [N,T,C,Ho,Wo]
    (cols * gcols.to(dtype).view(c.N, T, c.C, Ho, Wo)).sum().backward()
    return {"cols": cols.detach().reshape(c.N, T * c.C, Ho, Wo), "gx": leaves[0].grad, "goffset": leaves[1].grad,
            "gmask": leaves[2].grad if mask is not None else None}


@functools.lru_cache(maxsize=None)
def reference(c):
    """{quantity: (ref64, ref32)}, computed once per case and never written to"""
    x, off, mask, gcols = make_inputs(c)
    r64, r32 = _oracle(c, x, off, mask, gcols, torch.float64), _oracle(c, x, off, mask, gcols, torch.float32)
    return {k: (r64[k], r32[k].double()) for k in r64 if r64[k] is not None}


def check(c, what, got, ref64, ref32, keep=None):
    """e_k <= 4 * e_32 + 2^-22, both relative to max|ref64|; keep: boolean mask of the entries compared (None: all)"""
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    assert bool(torch.isfinite(got).all()), "%s: %s is not finite" % (c.name, what)
    scale = float(ref64.abs().max())
    assert scale > 0.0
    dk, d32 = (got - ref64).abs(), (ref32 - ref64).abs()
    if keep is not None:
        dk, d32 = dk * keep, d32 * keep
    e_k, e_32 = float(dk.max()) / scale, float(d32.max()) / scale
    bound = TOL_FACTOR * e_32 + TOL_FLOOR
    print("DSAMPLE form=%s case=%s what=%s e_k=%.3e e_32=%.3e ratio=%s of_bound=%.2f" % (
        FORM_NAME[c.form], c.name, what, e_k, e_32, "%.2f" % (e_k / e_32) if e_32 > 0 else "-", e_k / bound))
    assert e_k <= bound, "%s: %s off by %.3e of its maximum; the float32 oracle by %.3e" % (c.name, what, e_k, e_32)


def query_form(c):
    from da_detect_amd import _C

    Ho, Wo = out_size(c)
    return _C.deform_sample_backward_form(c.N, c.H, c.W, c.C, c.kh, c.kw, c.stride, c.pad, c.dil, c.dg, Ho, Wo,
                                          workspace=c.workspace)


def _dev(t, device):
    return t.to(device).contiguous(memory_format=CL) if t is not None else None


# ---------------------------------------------------------------------------------------------------------------
# without a GPU: the case table itself, the oracles, the query
@pytest.mark.parametrize("c", GATHER_CASES + [c for c in OM_CASES + EXACT_CASES if c.form == GATHER], ids=lambda c: c.name)
def test_gather_cases_have_the_list_lengths_they_name_cpu(c):
    off = (_exact_offsets(c)[0] if c in EXACT_CASES else make_om(c)[1] if c in OM_CASES else make_inputs(c)[1])
    n = longest_list(c, off)
    kind, v = c.longest
    print("DSAMPLE case=%s longest list %d" % (c.name, n))
    assert {"le": n <= v, "eq": n == v, "ge": n >= v}[kind], "%s: longest list %d, wanted %s %d" % (c.name, n, kind, v)
    if kind == "le":
        assert n >= 2      # the lists are in use


def test_backward_cases_take_the_form_they_name_cpu():
    """dadet_deform_sample_backward_form is pure host code: the whole table is asked without a device"""
    for c in BACKWARD_CASES + OM_CASES + EXACT_CASES:
        assert query_form(c) == c.form, "%s runs form %d, its table entry names %d" % (c.name, query_form(c), c.form)
    # the conditions one by one, from the gather case (2, 64, 6, 5, k 3): channels per group, kernel extent, stride, workspace
    from da_detect_amd import _C, _lib
    assert _C.deform_sample_backward_form(2, 6, 5, 64, 3, 3, 1, 1, 1, 1, 6, 5) == GATHER
    assert _C.deform_sample_backward_form(2, 6, 5, 64, 3, 3, 1, 1, 1, 2, 6, 5) == LDS
    assert _C.deform_sample_backward_form(2, 6, 5, 64, 3, 3, 1, 1, 1, 1, 6, 5, workspace=False) == LDS
    assert _C.deform_sample_backward_form(2, 6, 5, 32, 3, 3, 1, 1, 1, 1, 6, 5) == PLAIN
    assert _C.deform_sample_backward_form(2, 6, 5, 64, 3, 3, 2, 1, 1, 1, 3, 3) == PLAIN
    assert _C.deform_sample_backward_form(2, 6, 5, 64, 3, 3, 1, 2, 2, 1, 6, 5) == PLAIN
    assert _C.deform_sample_backward_form(2, 6, 5, 64, 1, 3, 1, 1, 1, 1, 8, 5) == GATHER
    lib = _lib.load()
    need = ctypes.c_size_t(0)
    assert lib.dadet_deform_sample_backward_workspace_bytes(2, 6, 5, 1, ctypes.byref(need)) == 0
    geom = (2, 6, 5, 64, 3, 3, 1, 1, 1, 1, 6, 5)
    assert lib.dadet_deform_sample_backward_form(*geom, need) == GATHER
    assert lib.dadet_deform_sample_backward_form(*geom, ctypes.c_size_t(need.value - 1)) == LDS      # too small a workspace
    assert lib.dadet_deform_sample_backward_form(2, 6, 5, 64, 3, 3, 1, 1, 1, 1, 7, 5, need) == -1      # Ho does not match
    with pytest.raises(_lib.DadetError):
        _C.deform_sample_backward_form(2, 6, 5, 2, 3, 3, 1, 1, 1, 1, 6, 5)


def test_fewer_than_four_channels_are_refused_on_the_host_cpu():
    """C = 2 and C = 0 are refused by the geometry check of forward and backward before anything is computed from C
    (the forward used to take a remainder by C / 4 first); the calls carry no pointers: nothing is launched"""
    from da_detect_amd import _lib

    lib = _lib.load()
    for C in (2, 0):
        geom = (1, 4, 4, C, 1, 1, 1, 0, 1, 1, 4, 4)
        assert lib.dadet_deform_sample_forward(None, None, None, None, *geom, None) != 0
        assert b"deform_sample_forward" in lib.dadet_last_error()
        assert lib.dadet_deform_sample_forward_ld(None, None, 2, None, 1, 0, None, *geom, None) != 0
        assert lib.dadet_deform_sample_backward(None, None, None, None, None, None, None, *geom, None) != 0
        assert b"deform_sample_backward" in lib.dadet_last_error()
        assert lib.dadet_deform_sample_backward_form(*geom, ctypes.c_size_t(0)) == -1
    assert lib.dadet_deform_sample_forward(None, None, None, None, 0, 4, 4, 4, 1, 1, 1, 0, 1, 1, 4, 4, None) == 0   # N = 0


def test_oracle_in_float32_is_close_to_float64_cpu():
    """the yardstick of the tolerance: on these inputs the float32 oracle stays within float32 rounding of float64 for
    every quantity (no sum here has more than 4 corners x 64 channels = 256 terms: n * 2^-24), so the bound
    4 * e_32 + 2^-22 is a rounding bound, not a loose one"""
    for c in (PLAIN_CASES[0], LDS_CASES[0], GATHER_CASES[0]):
        for what, (r64, r32) in reference(c).items():
            e_32 = float((r32 - r64).abs().max()) / float(r64.abs().max())
            print("DSAMPLE case=%s what=%s e_32=%.3e" % (c.name, what, e_32))
            assert e_32 <= 256 * 2.0 ** -24, (c.name, what, e_32)


# ---------------------------------------------------------------------------------------------------------------
# forward
@pytest.mark.gpu
@pytest.mark.parametrize("modulated", [False, True], ids=["v1", "v2"])
@pytest.mark.parametrize("c", FORWARD_CASES, ids=_ids(FORWARD_CASES))
def test_forward(device, c, modulated):
    from da_detect_amd import _C

    c = c._replace(modulated=modulated, name=c.name + ("_v2" if modulated else "_v1"))
    x, off, mask, _ = make_inputs(c)
    cols = _C.deform_sample_forward(_dev(x, device), _dev(off, device), _dev(mask, device), c.kh, c.kw, c.stride, c.pad,
                                    c.dil, c.dg)
    check(c, "cols", cols, *reference(c)["cols"])


@pytest.mark.gpu
def test_forward_of_an_empty_batch(device):
    from da_detect_amd import _C

    x = torch.empty((0, 8, 7, 9), device=device)
    off = torch.empty((0, 18, 7, 9), device=device)
    cols = _C.deform_sample_forward(x, off, None, 3, 3, 1, 1, 1, 1)
    assert cols.shape == (0, 72, 7, 9)


# ---------------------------------------------------------------------------------------------------------------
# backward, every form
def _backward(device, c, inputs=None):
    from da_detect_amd import _C

    x, off, mask, gcols = inputs if inputs is not None else make_inputs(c)
    return _C.deform_sample_backward(_dev(x, device), _dev(off, device), _dev(mask, device), _dev(gcols, device), c.kh, c.kw,
                                     c.stride, c.pad, c.dil, c.dg, need_x=c.need_x, workspace=c.workspace)


@pytest.mark.gpu
@pytest.mark.parametrize("c", BACKWARD_CASES, ids=_ids(BACKWARD_CASES))
def test_backward(device, c):
    assert query_form(c) == c.form
    if c.longest is not None:
        n = longest_list(c, make_inputs(c)[1])
        print("DSAMPLE case=%s longest list %d" % (c.name, n))
        assert {"le": n <= c.longest[1], "eq": n == c.longest[1], "ge": n >= c.longest[1]}[c.longest[0]]
    ref = reference(c)
    gx, goffset, gmask = _backward(device, c)
    if c.need_x:
        check(c, "gx", gx, *ref["gx"])
    else:
        assert gx is None
    check(c, "goffset", goffset, *ref["goffset"])
    if c.modulated:
        check(c, "gmask", gmask, *ref["gmask"])
    else:
        assert gmask is None
    if c.form == GATHER:
        # one writer per address and a fixed order inside it: the offset / modulation gradients are the same bits in every
        # run.  (gx is not: the order of a list, and of the overflow atomics, is the arrival order.)
        _, goffset2, gmask2 = _backward(device, c)
        assert torch.equal(goffset, goffset2)
        assert gmask is None or torch.equal(gmask, gmask2)


# ---------------------------------------------------------------------------------------------------------------
# offsets and modulation logits read in place from the offset conv's (padded) output
@functools.lru_cache(maxsize=None)
def make_om(c):
    """x, om [N, ld, Ho, Wo] (offsets, then logits with +-30 among them, then padding), gcols; ld = used channels padded to 4"""
    g = _gen(c, 1)
    Ho, Wo = out_size(c)
    T = c.kh * c.kw
    used = c.dg * T * (3 if c.modulated else 2)
    ld = (used + 3) & ~3
    x = torch.randn((c.N, c.C, c.H, c.W), generator=g)
    om = torch.randn((c.N, ld, Ho, Wo), generator=g) * 2        # the padding channels hold values nothing may read
    om[:, :2 * T * c.dg] = make_offsets(c, g)
    if c.modulated:
        lg = om[:, 2 * T * c.dg:used]
        pick = torch.rand(lg.shape, generator=g)
        lg[pick < 0.05] = 30.0       # saturated modulation: sigmoid = 1 in float32, mk * (1 - mk) = 0
        lg[pick > 0.95] = -30.0
    gcols = torch.randn((c.N, T * c.C, Ho, Wo), generator=g)
    return x, om, gcols


def _oracle_om(c, x, om, gcols, dtype):
    from oracle import deform_ref as R

    Ho, Wo = out_size(c)
    T = c.kh * c.kw
    x, om = x.to(dtype).clone().requires_grad_(True), om.to(dtype).clone().requires_grad_(True)
    off = om[:, :2 * T * c.dg]
    mask = om[:, 2 * T * c.dg:3 * T * c.dg].sigmoid() if c.modulated else None
    cols = R.deform_sample(x, off, mask, c.kh, c.kw, c.stride, c.pad, c.dil, c.dg)
    (cols * gcols.to(dtype).view(c.N, T, c.C, Ho, Wo)).sum().backward()
    return {"cols": cols.detach().reshape(c.N, T * c.C, Ho, Wo), "gx": x.grad, "gom": om.grad}


@pytest.mark.gpu
@pytest.mark.parametrize("c", OM_CASES, ids=_ids(OM_CASES))
def test_om_forms(device, c):
    from da_detect_amd import _C, amax

    assert query_form(c) == c.form
    x, om, gcols = make_om(c)
    T = c.kh * c.kw
    used = c.dg * T * (3 if c.modulated else 2)
    assert om.shape[1] > used, "the case is meant to have padding channels"
    r64, r32 = _oracle_om(c, x, om, gcols, torch.float64), _oracle_om(c, x, om, gcols, torch.float32)
    xd, omd, gd = _dev(x, device), _dev(om, device), _dev(gcols, device)
    cols = _C.deform_sample_forward_om(xd, omd, c.kh, c.kw, c.stride, c.pad, c.dil, c.dg, c.modulated)
    check(c, "om:cols", cols, r64["cols"], r32["cols"].double())
    gx, gom = _C.deform_sample_backward_om(xd, omd, gd, c.kh, c.kw, c.stride, c.pad, c.dil, c.dg, c.modulated,
                                           workspace=c.workspace)
    check(c, "om:gx", gx, r64["gx"], r32["gx"].double())
    check(c, "om:gom", gom, r64["gom"], r32["gom"].double())
    assert float(gom[:, used:].abs().max()) == 0.0, "padding channels of gom"
    assert _C.get_gemm_mode() == 4, "the suite runs in the default contraction mode 4, where the slot exists"
    got = amax.value(gom)
    assert got is not None and got == float(gom.abs().max()) and got > 0.0
    # the dense form on the sliced tensors (sigmoid applied outside): the same numbers, to the tolerance
    off_d = omd[:, :2 * T * c.dg].contiguous(memory_format=CL)
    mk_d = omd[:, 2 * T * c.dg:used].sigmoid().contiguous(memory_format=CL) if c.modulated else None
    gx_d, goff_d, gmk_d = _C.deform_sample_backward(xd, off_d, mk_d, gd, c.kh, c.kw, c.stride, c.pad, c.dil, c.dg,
                                                    workspace=c.workspace)
    dense = torch.zeros_like(r64["gom"])
    dense[:, :2 * T * c.dg] = goff_d.cpu().double()
    if c.modulated:
        mk = om[:, 2 * T * c.dg:used].double().sigmoid()
        dense[:, 2 * T * c.dg:used] = gmk_d.cpu().double() * mk * (1 - mk)
    for what, a, b, r in (("gx", gx, gx_d, "gx"), ("gom", gom, dense, "gom")):
        scale = float(r64[r].abs().max())
        e_32 = float((r32[r].double() - r64[r]).abs().max()) / scale
        diff = float((a.cpu().double() - b.cpu().double()).abs().max()) / scale
        print("DSAMPLE form=%s case=%s what=om-vs-dense:%s diff=%.3e e_32=%.3e" % (FORM_NAME[c.form], c.name, what, diff, e_32))
        assert diff <= TOL_FACTOR * e_32 + TOL_FLOOR, (what, diff, e_32)


# ---------------------------------------------------------------------------------------------------------------
# positions exactly on integers and exactly on the limits
def _exact_offsets(c):
    """the case's offsets with four taps of every pixel and group moved: tap 0 exactly on integer positions (both axes), tap 1
    exactly on h = -1 (contributes nothing), tap 2 exactly on w = W (nothing), tap 3 exactly on h = H - 1 (the last row alone).
    -> offsets, exact [N, dg*2*T, Ho, Wo] bool: the offset-gradient entries of those samples"""
    x, off, mask, gcols = make_inputs(c)
    T = c.kh * c.kw
    ys, xs = _base(c)
    off = off.double().clone()
    exact = torch.zeros(off.shape, dtype=torch.bool)
    for grp in range(c.dg):
        b = grp * 2 * T
        off[:, b + 0] = torch.floor(off[:, b + 0])
        off[:, b + 1] = torch.floor(off[:, b + 1])
        off[:, b + 2] = -1.0 - (ys + (1 // c.kw) * c.dil)
        off[:, b + 5] = float(c.W) - (xs + (2 % c.kw) * c.dil)
        off[:, b + 6] = float(c.H - 1) - (ys + (3 // c.kw) * c.dil)
        exact[:, b:b + 8] = True
    return off.float(), exact


@pytest.mark.gpu
@pytest.mark.parametrize("c", EXACT_CASES, ids=_ids(EXACT_CASES))
def test_exact_positions(device, c):
    """samples exactly on integer positions, exactly on h = -1 and on w = W (outside: they contribute nothing) and exactly
    on h = H - 1.  cols, gx and gmask are compared in full.  The bilinear kernel has a kink at an integer coordinate, where
    kernel and autograd may each take either one-sided derivative: the offset gradients of THOSE samples (both components),
    and only of those, are left out of the goffset comparison"""
    from da_detect_amd import _C

    assert query_form(c) == c.form
    x, _, mask, gcols = make_inputs(c)
    off, exact = _exact_offsets(c)
    r64, r32 = _oracle(c, x, off, mask, gcols, torch.float64), _oracle(c, x, off, mask, gcols, torch.float32)
    # the samples on h = -1 and w = W are outside in the reference too
    T = c.kh * c.kw
    for tap in (1, 2):
        assert float(r64["cols"].view(c.N, T, c.C, -1)[:, tap].abs().max()) == 0.0
    cols = _C.deform_sample_forward(_dev(x, device), _dev(off, device), _dev(mask, device), c.kh, c.kw, c.stride, c.pad,
                                    c.dil, c.dg)
    check(c, "exact:cols", cols, r64["cols"], r32["cols"].double())
    gx, goffset, gmask = _backward(device, c, (x, off, mask, gcols))
    check(c, "exact:gx", gx, r64["gx"], r32["gx"].double())
    check(c, "exact:gmask", gmask, r64["gmask"], r32["gmask"].double())
    check(c, "exact:goffset", goffset, r64["goffset"], r32["goffset"].double(), keep=~exact)
    # outside samples get no offset gradient at all
    T2 = 2 * T
    for grp in range(c.dg):
        assert float(goffset[:, grp * T2 + 2:grp * T2 + 4].abs().max()) == 0.0
        assert float(goffset[:, grp * T2 + 4:grp * T2 + 6].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("C", [2, 0])
def test_fewer_than_four_channels_are_refused(device, C):
    from da_detect_amd import _C, _lib

    x = torch.zeros((1, C, 4, 4), device=device)
    off = torch.zeros((1, 2, 4, 4), device=device)
    gcols = torch.zeros((1, C, 4, 4), device=device)
    with pytest.raises(_lib.DadetError):
        _C.deform_sample_forward(x, off, None, 1, 1, 1, 0, 1, 1)
    with pytest.raises(_lib.DadetError):
        _C.deform_sample_backward(x, off, None, gcols, 1, 1, 1, 0, 1, 1)
    with pytest.raises(_lib.DadetError):
        _C.deform_sample_backward(x, off, None, gcols, 1, 1, 1, 0, 1, 1, workspace=False)
