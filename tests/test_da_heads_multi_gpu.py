"""The instance-tail kernels with per-image row segments (dadet_da_ins_tail_forward_n / _backward_n) and the triplet
kernels on [k,C,H,W] batches, called through their `_C` wrappers, against float64 torch on the CPU.

Bars, gates and the seed search are those of tests/test_da_heads_gpu.py (its module docstring derives them); the reference of
the instance tail is that file's `_ins_reference` with the consistency rows of ANY number of images: row j of image i is
compared with means[l][i], and the bound of g_means[l][i] is a sum over image i's rows."""
import ctypes
import hashlib
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

from test_da_heads_gpu import (CL, EPS32, FLOOR, GATE, INV_KEEP, U, _assert_gate_margin, _check, _five_times,
                               _ins_conditions, _ins_inputs, _ins_reference, _spread, _sum_bound, _triplet_reference, f32)

pytestmark = pytest.mark.gpu


def _row_image(rows_per_image):
    return torch.cat([torch.full((n,), i, dtype=torch.long) for i, n in enumerate(rows_per_image)]) \
        if sum(rows_per_image) else torch.zeros(0, dtype=torch.long)


def _ends(rows_per_image):
    return [sum(rows_per_image[:i + 1]) for i in range(len(rows_per_image))]


def _ins_inputs_n(seed, C, rows_per_image, Rb, L):
    """the inputs of test_da_heads_gpu._ins_inputs with means [L, images]; thousands of rows: means out of the sigmoids'
    reach (logits stay within +-3: sigmoid in [0.047, 0.953]), alternating sides"""
    g = torch.Generator().manual_seed(seed)
    Rc, NI = sum(rows_per_image), len(rows_per_image)
    R = Rb + Rc
    z = torch.randn(R, C, generator=g)
    z = torch.where(z > 0, z.abs() + GATE, -(z.abs() + GATE)).float()
    mask = torch.where(torch.rand(R, C, generator=g) < 0.5, INV_KEEP, 0.0).float()
    w3 = (torch.randn(C, generator=g) * (0.4 / math.sqrt(C))).float()
    b3 = torch.tensor([0.05])
    labels = (torch.rand(Rb, generator=g) < 0.5).float() if Rb else None
    if R > 1000:
        side = (torch.arange(L)[:, None] + torch.arange(NI)[None]) % 2
        means = torch.where(side == 0, 0.02, 0.98).float() + 0.01 * torch.rand(L, NI, generator=g)
    else:
        means = (0.15 + 0.7 * torch.rand(L, NI, generator=g)).float()
    h = torch.relu(z) * mask
    return z, mask, h.contiguous(), w3, b3, labels, means.contiguous()


def _ins_conditions_n(h, w3, b3, means, Rb, rows_per_image):
    ref = h.double() @ w3.double() + b3.double()
    if float(ref.abs().max()) > 3.0:
        return False
    if sum(rows_per_image):
        d = (means.double()[:, _row_image(rows_per_image)] - torch.sigmoid(ref[Rb:])[None]).abs()      # [L, Rc]
        if float(d.min()) < GATE:
            return False
    return True


def _ins_reference_n(z, mask, h, w3, b3, labels, means, lg, coef, Rb, rows_per_image):
    """test_da_heads_gpu._ins_reference, image index per row instead of (row >= n_src)"""
    R, C = h.shape
    Rc, NI, L = sum(rows_per_image), len(rows_per_image), means.shape[0]
    img = _row_image(rows_per_image)
    c0, c1 = float(coef[0]), float(coef[1])
    lgv = lg.clone().requires_grad_(True)
    mv = means.double().clone().requires_grad_(True)
    bce_sum = torch.zeros((), dtype=torch.float64)
    if Rb:
        bce_sum = F.binary_cross_entropy_with_logits(lgv[:Rb], labels.double(), reduction="sum")
    cst_sum = torch.zeros((), dtype=torch.float64)
    cst_leaves = 0.0
    sg = torch.sigmoid(lgv[Rb:])
    for l in range(L if Rc else 0):
        cst_sum = cst_sum + (mv[l][img] - sg).abs().sum()
        cst_leaves = cst_leaves + float((mv[l][img] + sg).detach().sum())
    loss = c0 * bce_sum + c1 * cst_sum
    out = {"BCE sum": (bce_sum.detach(), _sum_bound(Rb, bce_sum.detach())),
           "consistency sum": (cst_sum.detach(), _sum_bound(Rc * L, cst_leaves, 2))}
    gl, = torch.autograd.grad(loss, lgv, retain_graph=bool(Rc))
    zz = z.double().requires_grad_(True)
    w = w3.double().requires_grad_(True)
    b = b3.double().requires_grad_(True)
    h64 = torch.relu(zz) * mask.double()
    assert torch.equal(h64.detach(), h.double())
    g_z, g_w3, g_b3 = torch.autograd.grad(h64 @ w + b, (zz, w, b), gl)
    s = torch.sigmoid(lg)
    leaves = torch.zeros(R, dtype=torch.float64)
    if Rb:
        leaves[:Rb] = abs(c0) * (s[:Rb] + labels.double())
    if Rc:
        sd = torch.sign(means.double()[:, img] - s[Rb:][None])                  # [L, Rc]
        leaves[Rb:] = abs(c1) * sd.sum(0).abs() * (s[Rb:] + s[Rb:] * s[Rb:])
        g_means, = torch.autograd.grad(loss, mv)
        n_img = torch.tensor([float(n) for n in rows_per_image], dtype=torch.float64)
        count = torch.stack([(sd.abs() * (img == i)[None]).sum(1) for i in range(NI)], 1)      # [L, NI] non-zero signs
        out["g_means"] = (g_means, _sum_bound(n_img[None], abs(c1) * count))
    open_ = (h.double() != 0).double()
    out["g_z"] = (g_z, _sum_bound(1, leaves[:, None] * INV_KEEP * w3.double().abs()[None] * open_, 2) + FLOOR)
    out["g_w3"] = (g_w3, _sum_bound(R, (leaves[:, None] * h.double().abs()).sum(0), 2))
    out["g_b3"] = (g_b3, _sum_bound(R, leaves.sum(), 2).reshape(1))
    return out


INS_N_CASES = [
    # C, consistency rows per image, R_bce, levels
    (12, [3, 4], 7, 3),                          # baseline, two images
    (12, [2, 0, 4, 1], 7, 1),                    # an empty image
    (12, [0, 0, 7], 7, 16),                      # leading empties, most levels
    (1024, [5, 3, 1, 6], 15, 3),                 # widest C
    (260, [1, 1, 1, 1, 1, 1], 0, 5),             # null labels
    (12, [1] * 9, 9, 2),                         # nine images
    (8, [300, 212, 513, 1000, 26], 2051, 2),     # R = 4102 > 512 x 4 rows: the forward grid cap
    (8, [1025] * 4, 4100, 2),                    # R = 8200 > 256 x 16 rows: the backward grid cap
]


@pytest.mark.parametrize("C,rows,Rb,L", INS_N_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_ins_tail_n_against_float64(device, C, rows, Rb, L):
    from da_detect_amd import _C

    Rc = sum(rows)
    for seed in range(700 + C, 700 + C + 64):
        z, mask, h, w3, b3, labels, means = _ins_inputs_n(seed, C, rows, Rb, L)
        if _ins_conditions_n(h, w3, b3, means, Rb, rows):
            break
    else:
        raise AssertionError("no seed gives a reference clear of the switching points")
    _assert_gate_margin(h.double())
    dev = lambda v: v.to(device) if v is not None else None      # noqa: E731
    hd, wd, bd, ld, md = dev(h), dev(w3), dev(b3), dev(labels), dev(means)
    ends = _ends(rows)
    logits, sums = _C.da_ins_tail_forward_n(hd, wd, bd, ld, md, Rb, Rc, ends)
    h64 = h.double()
    _check("logits", logits, h64 @ w3.double() + b3.double(),
           (C + 2) * U * (h64.abs() @ w3.double().abs() + b3.double().abs()))
    coef = torch.tensor([0.7 / max(Rb, 1), -1.3 / (max(Rc, 1) * max(L, 1))])
    ref = _ins_reference_n(z, mask, h, w3, b3, labels, means, logits.double().cpu(), coef, Rb, rows)
    _check("BCE sum", sums[0], *ref["BCE sum"])
    _check("consistency sum", sums[1], *ref["consistency sum"])
    g_z, g_w3, g_b3, g_means = _C.da_ins_tail_backward_n(hd, wd, logits, ld, md, coef.to(device), INV_KEEP, Rb, Rc, ends)
    _check("g_z", g_z, *ref["g_z"])
    _check("g_w3", g_w3, *ref["g_w3"])
    _check("g_b3", g_b3, *ref["g_b3"])
    assert bool((g_z.cpu()[h == 0] == 0).all())
    assert tuple(g_means.shape) == (L, len(rows))
    _check("g_means", g_means, *ref["g_means"])
    empty = [i for i, n in enumerate(rows) if n == 0]
    assert not bool(g_means.cpu()[:, empty].any())               # an image without rows: exactly no gradient


# the two-image cases whose forward bits tests/golden/da_ins_tail_bits.json holds: name -> (seed, C, R_bce, R_cst, n_src, L)
INS_BITS_CASES = {
    "two_images": (312, 12, 7, 7, 3, 3),
    "n_src_0": (313, 12, 7, 7, 0, 3),                 # every consistency row is image 1's
    "n_src_all": (314, 12, 7, 7, 7, 3),               # every consistency row is image 0's
    "no_consistency_rows": (315, 12, 7, 0, 0, 3),     # means is None
    "no_bce_rows": (316, 12, 0, 7, 3, 3),             # labels is None
    "production_rows": (317, 1024, 512, 512, 256, 1),
}
# n_src outside 0 .. R_cst: name -> (the case it is run on, the n_src it is run with, the case whose bits it gives)
INS_BITS_OUTSIDE = {"n_src_above": ("n_src_all", 7 + 5, "n_src_all"), "n_src_negative": ("n_src_0", -2, "n_src_0")}


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def ins_bits(case, device, run):
    """-> {"logits": sha256, "sums": sha256} of run(h, w3, b3, labels, means, R_bce, R_cst, n_src) on the case's inputs"""
    seed, C, Rb, Rc, n_src, L = INS_BITS_CASES[case]
    _, _, h, w3, b3, labels, means = _ins_inputs(seed, C, Rb, Rc, n_src, L)
    dev = lambda v: v.to(device) if v is not None else None      # noqa: E731
    logits, sums = run(dev(h), dev(w3), dev(b3), dev(labels), dev(means), Rb, Rc, n_src)
    return {"logits": _sha(logits), "sums": _sha(sums)}


def _two_image_entries(device):
    """-> (forward, backward) with the arguments of `_C.da_ins_tail_forward` / `_backward`, calling the native two-image
    entries dadet_da_ins_tail_forward / _backward themselves, n_src as given: `_C` calls only the `_n` entries, and gives
    the two-image wrappers their ends through its own `two_image_ends`"""
    from da_detect_amd import _C, _lib
    p, st = _C._p, _C._stream()

    def forward(h, w3, b3, labels, means, Rb, Rc, n_src):
        logits, sums = torch.empty(Rb + Rc, device=device), torch.zeros(2, device=device)
        _lib.call("dadet_da_ins_tail_forward", p(h), p(w3), p(b3), p(labels), p(means), p(logits), p(sums), Rb, Rc, n_src,
                  means.shape[0] if means is not None else 0, h.shape[1], st)
        return logits, sums

    def backward(h, w3, logits, labels, means, coef, inv_keep, Rb, Rc, n_src):
        C, L = h.shape[1], means.shape[0] if means is not None else 0
        g_z, g_w3, g_b3 = torch.empty_like(h), torch.zeros(C, device=device), torch.zeros(1, device=device)
        g_means = torch.zeros(L, 2, device=device) if L else None
        _lib.call("dadet_da_ins_tail_backward", p(h), p(w3), p(logits), p(labels), p(means), p(coef), inv_keep, p(g_z),
                  p(g_w3), p(g_b3), p(g_means), Rb, Rc, n_src, L, C, st)
        return g_z, g_w3, g_b3, g_means

    return forward, backward


def test_ins_tail_n_two_images_gives_the_old_entry_bits(device):
    """The two-image entries' kernels are gone: dadet_da_ins_tail_forward builds the table {clamp(n_src, 0, R_cst), R_cst}
    and launches the kernel of the `_n` entry.  What they wrote is kept as bits: the SHA-256 of logits and of both sums that
    the two-image entry gave at the last commit where it had kernels of its own, on an MI355X, twice
    (tests/golden/da_ins_tail_bits.json).  The native two-image entry, called directly, the two-image wrapper and the `_n`
    wrapper with [n_src, R_cst] all give them — same grid, same order of every sum — and an n_src above R_cst / below 0
    gives what R_cst / 0 gives, through the native entry's clamp and through the wrapper's."""
    from da_detect_amd import _C

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "da_ins_tail_bits.json")) as f:
        recorded = json.load(f)
    assert sorted(recorded["hashes"]) == sorted(INS_BITS_CASES) and recorded["not_reproducible"] == []
    native_forward, _ = _two_image_entries(device)
    for case in INS_BITS_CASES:
        assert ins_bits(case, device, native_forward) == recorded["hashes"][case], case
        assert ins_bits(case, device, _C.da_ins_tail_forward) == recorded["hashes"][case], case
        assert ins_bits(case, device, lambda *a: _C.da_ins_tail_forward_n(*a[:-1], [a[-1], a[-2]])) \
            == recorded["hashes"][case], case
    for on, n_src, gives in INS_BITS_OUTSIDE.values():
        for run in (native_forward, _C.da_ins_tail_forward):
            assert ins_bits(on, device, lambda *a: run(*a[:-1], n_src)) == recorded["hashes"][gives], n_src
    _, C, Rb, Rc, n_src, L = INS_BITS_CASES["two_images"]
    _, _, h, w3, b3, labels, means = _ins_inputs(312, C, Rb, Rc, n_src, L)
    new = _C.da_ins_tail_forward_n(*(v.to(device) for v in (h, w3, b3, labels, means)), Rb, Rc, [n_src, Rc])
    assert float(new[1][1]) > 0.0
    # thousands of rows, magnitudes over six decades: the workgroups' partial sums are added in one order
    g = torch.Generator().manual_seed(72)
    Rb, rows, C = 1025, [200, 0, 413, 413], 8
    Rc = sum(rows)
    hs = (_spread((Rb + Rc, C), g).abs() * (torch.rand(Rb + Rc, C, generator=g) < 0.5)).float().to(device)
    w3 = torch.randn(C, generator=g).to(device)
    labels = (torch.rand(Rb, generator=g) < 0.5).float().to(device)
    means = torch.rand(2, 4, generator=g).to(device)
    b3 = torch.tensor([0.05], device=device)
    _five_times(lambda: _C.da_ins_tail_forward_n(hs, w3, b3, labels, means, Rb, Rc, _ends(rows)))


@pytest.mark.parametrize("n_src", [3, 7 + 5, -2], ids=lambda v: "n_src=" + str(v))
def test_ins_tail_two_image_entries_against_float64(device, n_src):
    """dadet_da_ins_tail_forward / _backward called directly, C = 12 and 7 + 7 rows, with n_src inside, above and below
    0 .. R_cst: the float64 reference and bounds of test_da_heads_gpu.test_ins_tail_against_float64, whose row image is
    (row >= n_src) for ANY n_src — no clamp on the reference's side"""
    C, Rb, Rc, L = 12, 7, 7, 3
    for seed in range(300 + C, 300 + C + 64):
        z, mask, h, w3, b3, labels, means = _ins_inputs(seed, C, Rb, Rc, n_src, L)
        if _ins_conditions(h, w3, b3, means, Rb, Rc, n_src, False):
            break
    else:
        raise AssertionError("no seed gives a reference clear of the switching points")
    _assert_gate_margin(h.double())
    forward, backward = _two_image_entries(device)
    hd, wd, bd, ld, md = (v.to(device) for v in (h, w3, b3, labels, means))
    logits, sums = forward(hd, wd, bd, ld, md, Rb, Rc, n_src)
    h64 = h.double()
    _check("logits", logits, h64 @ w3.double() + b3.double(),
           (C + 2) * U * (h64.abs() @ w3.double().abs() + b3.double().abs()))
    coef = torch.tensor([0.7 / Rb, -1.3 / (Rc * L)])
    ref = _ins_reference(z, mask, h, w3, b3, labels, means, logits.double().cpu(), coef, Rb, Rc, n_src)
    _check("BCE sum", sums[0], *ref["BCE sum"])
    _check("consistency sum", sums[1], *ref["consistency sum"])
    g_z, g_w3, g_b3, g_means = backward(hd, wd, logits, ld, md, coef.to(device), INV_KEEP, Rb, Rc, n_src)
    for name, g in (("g_z", g_z), ("g_w3", g_w3), ("g_b3", g_b3), ("g_means", g_means)):
        _check(name, g, *ref[name])
    assert bool((g_z.cpu()[h == 0] == 0).all())
    if not 0 < n_src < Rc:
        assert not bool(g_means.cpu()[:, 0 if n_src <= 0 else 1].any())      # the image without rows: exactly no gradient


def test_ins_tail_n_refusals_write_nothing(device):
    """ends not ascending; last end != R_cst; 0 and 65 images; more levels x images than the backward keeps in LDS (512):
    DadetError, and every output buffer keeps its fill"""
    from da_detect_amd import _C, _lib

    C, Rb, Rc = 8, 3, 6
    p, st = _C._p, _C._stream()
    h = torch.ones((Rb + Rc, C), device=device)
    w3, b3 = torch.ones(C, device=device), torch.ones(1, device=device)
    labels = torch.ones(Rb, device=device)
    coef = torch.ones(2, device=device)

    def both(ends, n_img, levels, forward_refuses=True):
        means = torch.full((max(levels * max(n_img, 1), 1),), 0.5, device=device)
        outs = [torch.full(s, 7.0, device=device) for s in ((Rb + Rc,), (2,), (Rb + Rc, C), (C,), (1,), (means.numel(),))]
        lg, sm, gz, gw, gb, gm = outs
        arr = (ctypes.c_int * max(len(ends), 1))(*ends)
        fwd = lambda: _lib.call("dadet_da_ins_tail_forward_n", p(h), p(w3), p(b3), p(labels), p(means), p(lg), p(sm),  # noqa
                                Rb, Rc, arr, n_img, levels, C, st)
        if forward_refuses:
            with pytest.raises(_lib.DadetError):
                fwd()
        with pytest.raises(_lib.DadetError):
            _lib.call("dadet_da_ins_tail_backward_n", p(h), p(w3), p(lg), p(labels), p(means), p(coef), 2.0, p(gz), p(gw),
                      p(gb), p(gm), Rb, Rc, arr, n_img, levels, C, st)
        torch.cuda.synchronize()
        for o in (outs if forward_refuses else outs[2:]):
            assert bool((o == 7.0).all())

    both([4, 2, 6], 3, 1)                    # not ascending
    both([-1, 6], 2, 1)                      # a negative end
    both([2, 5], 2, 1)                       # last end != R_cst
    both([2, 7], 2, 1)
    both([], 0, 1)                           # no image
    both(list(range(0, 65)), 65, 1)          # one image too many for the by-value table
    # 16 levels x 33 images = 528 sums: the forward keeps nothing per image and runs, the backward refuses
    both([0] * 32 + [Rc], 33, 16, forward_refuses=False)
    # the wrappers pass the same refusals on
    with pytest.raises(_lib.DadetError):
        _C.da_ins_tail_forward_n(h, w3, b3, labels, torch.full((1, 2), 0.5, device=device), Rb, Rc, [5, 6][::-1])


# ============================================================================================== triplet, k images
def _triplet_inputs_k(seed, k, C, H, W):
    g = torch.Generator().manual_seed(seed)
    a, p, n = (torch.randn(k, C, H, W, generator=g) for _ in range(3))
    if C * H >= 4:             # in the LAST image: one (h, c) whose positive sits at a + eps: d_ap == 0 exactly, hinge active
        a[k - 1, 0, 0, :] = 0.0
        p[k - 1, 0, 0, :] = EPS32
        n[k - 1, 0, 0, :] = 0.02 * torch.randn(W, generator=g)
    return a, p, n


@pytest.mark.parametrize("k,C,H,W", [(4, 1, 1, 1), (2, 3, 5, 7), (3, 64, 9, 13), (2, 100, 3, 1)], ids=lambda v: str(v))
def test_triplet_batch_against_float64(device, k, C, H, W):
    """triplet_w_forward / _backward on [k,C,H,W] against nn.TripletMarginLoss(margin, p=2, eps) in float64 and its autograd:
    the bounds of test_triplet_against_float64 (its `_triplet_reference` takes any leading dimension), the hinge sum over
    k H C terms, the mean's divisor k H C; and through the autograd wrapper the loss and three gradients of the mean"""
    from da_detect_amd import _C
    from da_detect_amd.modeling.da_heads.fused import triplet_margin_loss_w

    margin = 0.25
    many = C * H >= 4
    terms = k * C * H
    for seed in range(800 + C, 800 + C + 64):
        a, p, n = _triplet_inputs_k(seed, k, C, H, W)
        g_scale = f32(0.7 / terms)
        ref = _triplet_reference(a, p, n, margin, g_scale)
        both_sides = bool(ref["active"].any()) and not bool(ref["active"].all())
        if float(ref["hinge"].abs().min()) >= GATE and (both_sides or not many):
            break
    else:
        raise AssertionError("no seed gives a reference clear of the switching points")
    assert ref["hinge"].numel() == terms
    if many:
        assert float(ref["dap"][k - 1, 0, 0]) == 0.0 and bool(ref["active"][k - 1, 0, 0])
    ad, pd, nd = (v.to(device).contiguous(memory_format=CL) for v in (a, p, n))
    loss, dist = _C.triplet_w_forward(ad, pd, nd, margin)
    assert tuple(dist.shape) == (terms, 2)
    dist4 = dist.view(k, H, C, 2)
    _check("d_ap", dist4[..., 0], ref["dap"].permute(0, 2, 1), ref["b_dap"].permute(0, 2, 1))
    _check("d_an", dist4[..., 1], ref["dan"].permute(0, 2, 1), ref["b_dan"].permute(0, 2, 1))
    _check("loss", loss, (ref["loss_sum"] / terms).reshape(1), ref["b_loss"] / terms)
    gsd = torch.tensor([g_scale], device=device)
    got = _C.triplet_w_backward(ad, pd, nd, dist, gsd, margin)
    for name, g in zip(("ga", "gp", "gn"), got):
        assert tuple(g.shape) == (k, C, H, W)
        _check(name, g, *ref[name])
        off = ~ref["active"][..., None].expand(k, C, H, W)
        assert not bool(g.cpu()[off].any())                   # inactive hinge: exactly zero
    if many:
        assert not bool(got[1][k - 1, 0, 0].any())            # d_ap == 0: no gradient for p, as float64 torch
    # the autograd wrapper: mean over (k, C, H); upstream gradient 0.7 -> g_scale = 0.7 / (k C H), the value used above
    av, pv, nv = (v.clone().requires_grad_(True) for v in (ad, pd, nd))
    out = triplet_margin_loss_w(av, pv, nv, margin)
    assert torch.equal(out.reshape(1), loss.reshape(1))
    (0.7 * out).backward()
    for name, leaf in zip(("ga", "gp", "gn"), (av, pv, nv)):
        _check(name + " (autograd)", leaf.grad, *ref[name])
    with pytest.raises(ValueError):
        triplet_margin_loss_w(ad, pd[:1], nd, margin)
