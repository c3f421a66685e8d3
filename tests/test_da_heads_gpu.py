"""The fused DA-head kernels of csrc/da_heads.hip called directly through their `_C` wrappers, against float64 torch on the
CPU, at the shapes where a kernel can go wrong: channel widths that are no multiple of a wavefront's float4 sweep, few rows,
rows past every launch's grid cap (the second trip of the grid-stride loops), 8 and 9 images, empty launches, null label /
mean pointers, and the refusals of the backward entry points.

Bars.  u = 2^-24.  Two steps, so that each error source has a bound of its own:
  1. logits against float64:  |got - ref| <= (C + 2) u (sum_c |x_c w_c| + |b|), the bound of a length-C fp32 dot product
     summed in any order.
  2. everything after the logit against a float64 reference evaluated AT THE KERNEL'S OWN fp32 logits (gradients from
     float64 autograd, never from a formula written out here):
       a value that is one chain of multiplications / divisions:  16 u |ref|  + one fp32 denormal step;
       a sum of n values:  (n + 2) u S + 16 u S,  S = sum of |terms| of the reference.
     Where a value is itself a signed combination of k leaf terms (s - y;  s (1 - s) = s - s^2;
     a_bce (s - y) + a_sig s (1 - s);  |mean - s|;  the triplet's a - p + eps and dp - dn), rounding of one leaf is not
     small against the combination, so S is taken over the LEAVES and the k - 1 additions inside a value count like the
     n - 1 between values:
       (n + k + 1 + 16) u S                                  (k = 1 is the plain sum bound above).
     The 16 u covers the handful of fp32 operations and the expf / logf calls per leaf.  No case needed more.
Inputs are seeded and chosen so that the float64 reference alone keeps every ReLU / dropout gate, every sign of
mean - sigmoid and every hinge at least 1e-3 away from its switching point, and BCE logits within +-3 (ATen's
log(exp(-m) + exp(-x - m)) loses the small term's bits against the 1 beyond that, with few rows to average over); the tests
assert these conditions on the reference.  Where a condition is a matter of chance (a few hundred draws against a 2e-3
window) the inputs are drawn again from the next seed until the reference satisfies it.

Forward loss sums are formed in a fixed order and must be bit-stable from run to run; the four atomically summed parameter
gradients (g_w2, g_b2, g_w3, g_b3) and g_means are not, and are only held to the bounds.

Every check prints its largest err / bound ratio."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
CL = torch.channels_last
U = 2.0 ** -24
FLOOR = 2.0 ** -149                      # one fp32 denormal step
EPS32 = float(np.float32(1e-6))          # the eps the triplet kernel adds: 1e-6 rounded to fp32
GATE = 1e-3
INV_KEEP = 2.0


def f32(v):
    return float(np.float32(v))


def _check(name, got, ref, bound):
    got = got.detach().to("cpu", torch.float64)
    ref = ref.detach().to(torch.float64)
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), name + ": non-finite"
    bound = torch.as_tensor(bound, dtype=torch.float64).broadcast_to(ref.shape)
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)       # a zero bound admits only the exact value
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print("    %-30s max err / bound = %.4f   (n = %d)" % (name, worst, ratio.numel()))
    assert worst <= 1.0, "%s: err / bound = %.3f" % (name, worst)
    return worst


def _elem_bound(ref):
    return 16 * U * ref.abs() + FLOOR


def _sum_bound(n, abs_sum, leaves=1):
    return (n + leaves + 1 + 16) * U * abs_sum


def _gated(z):
    """randn -> exactly 0 where z <= 0, |z| + 1e-3 elsewhere: a post-ReLU map whose open units are >= 1e-3"""
    return torch.where(z > 0, z.abs() + GATE, torch.zeros(())).float()


def _assert_gate_margin(x):
    nz = x[x != 0]
    assert nz.numel() == 0 or float(nz.abs().min()) >= GATE


def _spread(shape, g):
    """magnitudes over about six decades: another order of summation rounds differently"""
    return torch.randn(shape, generator=g) * 10.0 ** (torch.rand(shape, generator=g) * 6 - 3)


# ======================================================================================================== image head
def _img_inputs(seed, N, HW, C1):
    g = torch.Generator().manual_seed(seed)
    t = _gated(torch.randn(N * HW, C1, generator=g))
    w2 = (torch.randn(C1, generator=g) * (0.4 / math.sqrt(0.5 * C1))).float()
    b2 = torch.tensor([0.1])
    labels = (torch.arange(N) % 2 == 0).float()
    return t, w2, b2, labels


def _img_check_forward(got_logits, got_sums, t, w2, b2, labels, N, HW):
    t64, w64, b64 = t.double(), w2.double(), b2.double()
    _assert_gate_margin(t64)
    ref = t64 @ w64 + b64
    assert float(ref.abs().max()) <= 3.0
    C1 = w2.numel()
    _check("logits", got_logits, ref, (C1 + 2) * U * (t64.abs() @ w64.abs() + b64.abs()))
    lg = got_logits.double().cpu()
    ref_sums = torch.zeros(N, 2, dtype=torch.float64)
    for i in range(N):
        rows = lg[i * HW:(i + 1) * HW]
        ref_sums[i, 0] = F.binary_cross_entropy_with_logits(rows, labels[i].double().expand(HW), reduction="sum")
        ref_sums[i, 1] = torch.sigmoid(rows).sum()
    _check("BCE sum per image", got_sums[:, 0], ref_sums[:, 0], _sum_bound(HW, ref_sums[:, 0]))
    _check("sigmoid sum per image", got_sums[:, 1], ref_sums[:, 1], _sum_bound(HW, ref_sums[:, 1]))


def _img_ref_backward(t, w2, b2, labels, lg, coef, N, HW):
    """float64 autograd in two stages: d loss / d logit at the kernel's own logits, then through relu(z) @ w + b.
    coef [N, 4] (fp32 values) = (a_bce_w, a_sig_w, a_bce_x, a_sig_x) as include/dadet.h documents them.
    -> dict name -> (reference, bound)"""
    M = N * HW
    img = torch.arange(M) // HW
    cf = coef.double()[img]
    y = labels.double()[img]
    lgv = lg.clone().requires_grad_(True)
    bce = F.binary_cross_entropy_with_logits(lgv, y, reduction="none")
    sg = torch.sigmoid(lgv)
    gl_w, = torch.autograd.grad((cf[:, 0] * bce + cf[:, 1] * sg).sum(), lgv, retain_graph=True)
    gl_x, = torch.autograd.grad((cf[:, 2] * bce + cf[:, 3] * sg).sum(), lgv)
    t64 = t.double()
    z = torch.where(t64 > 0, t64, -torch.ones(())).requires_grad_(True)        # relu(z) == t, gate closed where t == 0
    w = w2.double().requires_grad_(True)
    b = b2.double().requires_grad_(True)
    logit = torch.relu(z) @ w + b
    g_t_w, g_w2, g_b2 = torch.autograd.grad(logit, (z, w, b), gl_w, retain_graph=True)
    g_t_x, = torch.autograd.grad(logit, z, gl_x)
    s = sg.detach()
    leaves_w = cf[:, 0].abs() * (s + y) + cf[:, 1].abs() * (s + s * s)          # 4 leaves per row
    leaves_x = cf[:, 2].abs() * (s + y) + cf[:, 3].abs() * (s + s * s)
    gate = (t64 > 0).double()
    wabs = w2.double().abs()
    return {
        "g_t_w": (g_t_w, _sum_bound(1, leaves_w[:, None] * wabs[None] * gate, 4) + FLOOR),
        "g_t_x": (g_t_x, _sum_bound(1, leaves_x[:, None] * wabs[None] * gate, 4) + FLOOR),
        "g_w2": (g_w2, _sum_bound(M, (leaves_w[:, None] * t64).sum(0), 4)),
        "g_b2": (g_b2, _sum_bound(M, leaves_w.sum(), 4).reshape(1)),
    }


def _img_coef(N, HW):
    k = torch.linspace(-0.7, 0.9, N) if N > 1 else torch.tensor([0.3])
    a_bce = torch.full((N,), 1.0 / (N * HW))
    a_sig = k / HW
    return torch.stack([a_bce, a_sig, -0.1 * a_bce, 0.3 * a_sig], 1).float().contiguous()


def _img_check_backward(got, ref):
    for name, g in zip(("g_t_w", "g_t_x", "g_w2", "g_b2"), got):
        _check(name, g, *ref[name])
    closed = ref["g_t_w"][0] == 0
    assert bool((got[0].cpu()[closed] == 0).all()) and bool((got[1].cpu()[closed] == 0).all())


IMG_CASES = [
    # num_images, rows_per_image, C1
    (2, 37, 4), (2, 37, 252), (2, 37, 256), (2, 37, 260), (2, 37, 1024),       # idle lanes in the last float4 sweep
    (1, 1, 8),                  # one active wavefront
    (3, 5, 8),                  # a wavefront's rows cross two image boundaries
    (2, 185, 512),              # the workload's kind of shape
    (2, 35001, 4),              # M > 2048 * 32 and > 1024 * 64: both grid caps, the second grid-stride trip
    (8, 5, 8),                  # the last LDS slot of the fixed-order path
    (9, 5, 8),                  # one image too many for it: atomics, no scratch
]


@pytest.mark.parametrize("N,HW,C1", IMG_CASES, ids=lambda v: str(v))
def test_img_head_against_float64(device, N, HW, C1):
    """da_img_head_loss_forward and da_img_head_loss_backward (the `coef` entry point); bounds of the module docstring,
    leaves per row of the backward: a_bce s, a_bce y, a_sig s, a_sig s^2."""
    from da_detect_amd import _C

    t, w2, b2, labels = _img_inputs(100 + N * 7 + C1, N, HW, C1)
    td, wd, bd, ld = (v.to(device) for v in (t, w2, b2, labels))
    logits, sums = _C.da_img_head_loss_forward(td, wd, bd, ld, N, HW)
    _img_check_forward(logits, sums, t, w2, b2, labels, N, HW)
    coef = _img_coef(N, HW)
    got = _C.da_img_head_loss_backward(td, wd, logits, ld, coef.to(device), N, HW)
    _img_check_backward(got, _img_ref_backward(t, w2, b2, labels, logits.double().cpu(), coef, N, HW))


def test_img_head_backward_refuses_more_than_1024_channels(device):
    """C1 = 1028: the forward's float4 sweep has no limit; a lane of the backward kernels owns four float4 slots, so both
    backward entry points refuse it"""
    from da_detect_amd import _C, _lib

    N, HW, C1 = 2, 9, 1028
    t, w2, b2, labels = _img_inputs(7, N, HW, C1)
    td, wd, bd, ld = (v.to(device) for v in (t, w2, b2, labels))
    logits, sums = _C.da_img_head_loss_forward(td, wd, bd, ld, N, HW)
    _img_check_forward(logits, sums, t, w2, b2, labels, N, HW)
    with pytest.raises(_lib.DadetError):
        _C.da_img_head_loss_backward(td, wd, logits, ld, _img_coef(N, HW).to(device), N, HW)
    with pytest.raises(_lib.DadetError):
        _C.da_img_head_loss_backward_g(td, wd, logits, ld, torch.ones(1, device=device), None, 0.1, 0.1, N, HW)


def test_img_head_zero_images_touches_nothing(device):
    from da_detect_amd import _C, _lib

    C1, HW = 8, 5
    empty = torch.empty((0, C1), device=device)
    w2, b2 = torch.ones(C1, device=device), torch.ones(1, device=device)
    logits, sums = _C.da_img_head_loss_forward(empty, w2, b2, torch.empty(0, device=device), 0, HW)
    assert tuple(logits.shape) == (0,) and tuple(sums.shape) == (0, 2)
    g_t_w, g_t_x, g_w2, g_b2 = _C.da_img_head_loss_backward(empty, w2, logits, torch.empty(0, device=device),
                                                            torch.empty((0, 4), device=device), 0, HW)
    assert g_t_w.numel() == 0 and not bool(g_w2.any()) and not bool(g_b2.any())
    # the library itself, on buffers it could write: every output keeps its fill
    t = torch.ones((2 * HW, C1), device=device)
    labels = torch.ones(2, device=device)
    outs = [torch.full(s, 7.0, device=device) for s in ((2 * HW,), (2, 2), (2 * HW, C1), (2 * HW, C1), (C1,), (1,))]
    lg, sm, gw, gx, gw2, gb2 = outs
    p, st = _C._p, _C._stream()
    _lib.call("dadet_da_img_head_loss_forward", p(t), p(w2), p(b2), p(labels), p(lg), p(sm), 0, HW, C1, st)
    _lib.call("dadet_da_img_head_loss_backward", p(t), p(w2), p(lg), p(labels), p(torch.ones((2, 4), device=device)), p(gw),
              p(gx), p(gw2), p(gb2), 0, HW, C1, st)
    _lib.call("dadet_da_img_head_loss_backward_gm", p(t), p(w2), p(lg), p(labels), p(b2), None, None, 0.5, 0.5, p(gw),
              p(gx), p(gw2), p(gb2), 0, HW, C1, None, None, st)
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == 7.0).all())


@pytest.mark.parametrize("adv_on_device", [False, True], ids=["float w_adv", "0-d device w_adv"])
@pytest.mark.parametrize("with_sig", [True, False], ids=["g_mean_sig", "no g_mean_sig"])
def test_img_head_backward_g_forms_the_same_coefficients(device, adv_on_device, with_sig):
    """da_img_head_loss_backward_g (the entry point the model uses) forms (g_bce / M, g_sig / HW, x w_adv, x w_cst) in the
    kernel: the same fp32 operations made here on the host give the `coef` form.  The two gradient maps agree within the
    elementwise bound, and all four outputs meet the float64 bounds.  need_x = False: no g_t_x, g_t_w bit for bit the same.
    Contraction mode 4: the slots travelling with g_t_w / g_t_x hold exactly their largest magnitudes."""
    from da_detect_amd import _C, amax

    N, HW, C1 = 3, 11, 260
    t, w2, b2, labels = _img_inputs(55, N, HW, C1)
    td, wd, bd, ld = (v.to(device) for v in (t, w2, b2, labels))
    logits, _ = _C.da_img_head_loss_forward(td, wd, bd, ld, N, HW)
    g_bce = torch.tensor([0.8])
    g_sig = torch.tensor([0.3, -0.7, 0.45]) if with_sig else None
    w_adv, w_cst = torch.tensor(-0.1), torch.tensor(0.3)                       # fp32 values
    cx = (g_bce / float(N * HW)).expand(N)
    cy = g_sig / float(HW) if with_sig else torch.zeros(N)
    coef = torch.stack([cx, cy, cx * w_adv, cy * w_cst], 1).contiguous()
    assert coef.dtype == torch.float32
    prev = _C.get_gemm_mode()
    try:
        _C.set_gemm_mode(4)
        adv = w_adv.to(device) if adv_on_device else float(w_adv)
        sig_d = g_sig.to(device) if with_sig else None
        got = _C.da_img_head_loss_backward_g(td, wd, logits, ld, g_bce.to(device), sig_d, adv, float(w_cst), N, HW)
        for g in got[:2]:
            assert amax.value(g) == float(g.abs().max()) > 0.0
        lean = _C.da_img_head_loss_backward_g(td, wd, logits, ld, g_bce.to(device), sig_d, adv, float(w_cst), N, HW,
                                              need_x=False)
        assert lean[1] is None and torch.equal(lean[0], got[0])
        assert amax.value(lean[0]) == float(lean[0].abs().max())
    finally:
        _C.set_gemm_mode(prev)
    _img_check_backward(got, _img_ref_backward(t, w2, b2, labels, logits.double().cpu(), coef, N, HW))
    by_coef = _C.da_img_head_loss_backward(td, wd, logits, ld, coef.to(device), N, HW)
    _check("g_t_w: _g against coef", got[0], by_coef[0].double().cpu(), _elem_bound(by_coef[0].double().cpu()))
    _check("g_t_x: _g against coef", got[1], by_coef[1].double().cpu(), _elem_bound(by_coef[1].double().cpu()))
    lean = _C.da_img_head_loss_backward(td, wd, logits, ld, coef.to(device), N, HW, need_x=False)
    assert lean[1] is None and torch.equal(lean[0], by_coef[0])


# ================================================================================================ instance head tail
FAR_MEANS = torch.tensor([[0.02, 0.98], [0.97, 0.03]])      # out of the sigmoids' reach: for thousands of rows


def _ins_inputs(seed, C, Rb, Rc, n_src, L, tie=False):
    g = torch.Generator().manual_seed(seed)
    R = Rb + Rc
    z = torch.randn(R, C, generator=g)
    z = torch.where(z > 0, z.abs() + GATE, -(z.abs() + GATE)).float()         # fc2 pre-activation
    mask = torch.where(torch.rand(R, C, generator=g) < 0.5, INV_KEEP, 0.0).float()
    w3 = (torch.randn(C, generator=g) * (0.4 / math.sqrt(C))).float()
    b3 = torch.tensor([0.0 if tie else 0.05])
    labels = (torch.rand(Rb, generator=g) < 0.5).float() if Rb else None
    means = None
    if Rc:
        means = FAR_MEANS[:L].clone() if R > 1000 else (0.15 + 0.7 * torch.rand(L, 2, generator=g)).float()
    if tie:
        z[Rb + 2] = -1.0                    # every unit of that row closed: h = 0, logit = b3 = 0, sigmoid = 0.5
        means[0, 0] = 0.5                   # its image's mean (row 2 < n_src): mean - sigmoid == 0 exactly
    h = torch.relu(z) * mask
    return z, mask, h.contiguous(), w3, b3, labels, means


def _ins_conditions(h, w3, b3, means, Rb, Rc, n_src, tie):
    h64 = h.double()
    ref = h64 @ w3.double() + b3.double()
    if float(ref.abs().max()) > 3.0:
        return False
    if Rc:
        img = (torch.arange(Rc) >= n_src).long()
        d = (means.double()[:, img] - torch.sigmoid(ref[Rb:])[None]).abs()      # [L, Rc]
        if tie:
            assert float(d[0, 2]) == 0.0
            d[0, 2] = 1.0
        if float(d.min()) < GATE:
            return False
    return True


def _ins_reference(z, mask, h, w3, b3, labels, means, lg, coef, Rb, Rc, n_src):
    """float64 autograd in two stages, as for the image head: the loss of include/dadet.h (coef[0] x BCE sum + coef[1] x
    consistency sum) at the kernel's own logits, then through (relu(z) * mask) @ w3 + b3.  Leaves per row: BCE rows
    a_bce s, a_bce y; consistency rows a_cst |sum of signs| (s, s^2)."""
    R, C = h.shape
    L = means.shape[0] if means is not None else 0
    c0, c1 = float(coef[0]), float(coef[1])
    lgv = lg.clone().requires_grad_(True)
    mv = means.double().clone().requires_grad_(True) if L else None
    bce_sum = torch.zeros((), dtype=torch.float64)
    if Rb:
        bce_sum = F.binary_cross_entropy_with_logits(lgv[:Rb], labels.double(), reduction="sum")
    cst_sum = torch.zeros((), dtype=torch.float64)
    cst_leaves = 0.0
    sg = torch.sigmoid(lgv[Rb:])
    img = (torch.arange(Rc) >= n_src).long()
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
        n_img = torch.tensor([float((img == 0).sum()), float((img == 1).sum())], dtype=torch.float64)
        count = torch.stack([(sd.abs() * (img == i)[None]).sum(1) for i in (0, 1)], 1)      # [L, 2] non-zero signs
        out["g_means"] = (g_means, _sum_bound(n_img[None], abs(c1) * count))
    open_ = (h.double() != 0).double()
    out["g_z"] = (g_z, _sum_bound(1, leaves[:, None] * INV_KEEP * w3.double().abs()[None] * open_, 2) + FLOOR)
    out["g_w3"] = (g_w3, _sum_bound(R, (leaves[:, None] * h.double().abs()).sum(0), 2))
    out["g_b3"] = (g_b3, _sum_bound(R, leaves.sum(), 2).reshape(1))
    return out


INS_CASES = [
    # C, R_bce, R_cst, n_src, levels, backward
    (4, 7, 7, 3, 3, True), (252, 7, 7, 3, 3, True), (260, 7, 7, 3, 3, True), (1024, 7, 7, 3, 3, True),
    (12, 7, 0, 0, 0, True), (12, 0, 7, 3, 1, True), (12, 1, 0, 0, 0, True),    # null means / null labels
    (12, 7, 7, 0, 1, True), (12, 7, 7, 7, 1, True),                            # every consistency row target / source
    (12, 7, 7, 3, 16, True),
    (8, 1025, 1026, 500, 2, True),       # R = 2051 > 512 x 4 rows: the forward grid cap
    (8, 2050, 2050, 1000, 2, True),      # R = 4100 > 256 x 16 rows: the backward grid cap
    (1028, 3, 3, 1, 1, False),           # forward only: the backward refuses C > 1024
    (12, 3, 3, 1, 17, False),            # forward only: the backward refuses more than 16 levels
]


@pytest.mark.parametrize("C,Rb,Rc,n_src,L,backward", INS_CASES, ids=lambda v: str(v))
def test_ins_tail_against_float64(device, C, Rb, Rc, n_src, L, backward):
    from da_detect_amd import _C, _lib

    for seed in range(300 + C, 300 + C + 64):
        z, mask, h, w3, b3, labels, means = _ins_inputs(seed, C, Rb, Rc, n_src, L)
        if _ins_conditions(h, w3, b3, means, Rb, Rc, n_src, False):
            break
    else:
        raise AssertionError("no seed gives a reference clear of the switching points")
    _assert_gate_margin(h.double())
    dev = lambda v: v.to(device) if v is not None else None      # noqa: E731
    hd, wd, bd, ld, md = dev(h), dev(w3), dev(b3), dev(labels), dev(means)
    logits, sums = _C.da_ins_tail_forward(hd, wd, bd, ld, md, Rb, Rc, n_src)
    h64 = h.double()
    _check("logits", logits, h64 @ w3.double() + b3.double(),
           (C + 2) * U * (h64.abs() @ w3.double().abs() + b3.double().abs()))
    coef = torch.tensor([0.7 / max(Rb, 1), -1.3 / (max(Rc, 1) * max(L, 1))])
    ref = _ins_reference(z, mask, h, w3, b3, labels, means, logits.double().cpu(), coef, Rb, Rc, n_src)
    _check("BCE sum", sums[0], *ref["BCE sum"])
    _check("consistency sum", sums[1], *ref["consistency sum"])
    if not backward:
        with pytest.raises(_lib.DadetError):
            _C.da_ins_tail_backward(hd, wd, logits, ld, md, coef.to(device), INV_KEEP, Rb, Rc, n_src)
        return
    g_z, g_w3, g_b3, g_means = _C.da_ins_tail_backward(hd, wd, logits, ld, md, coef.to(device), INV_KEEP, Rb, Rc, n_src)
    _check("g_z", g_z, *ref["g_z"])
    _check("g_w3", g_w3, *ref["g_w3"])
    _check("g_b3", g_b3, *ref["g_b3"])
    # dropout gate: zero exactly where the unit was dropped or closed, 1 / keep carried by every other one (the bound of
    # g_z is relative, so a missing factor 2 cannot pass it)
    assert bool((g_z.cpu()[h == 0] == 0).all())
    if Rc:
        _check("g_means", g_means, *ref["g_means"])
    else:
        assert g_means is None


def test_ins_tail_exact_tie_adds_nothing(device):
    """one consistency row with h = 0, b3 = 0 and its image's mean at 0.5: logit 0, sigmoid exactly 0.5, mean - sigmoid
    exactly 0.  torch's abs has gradient 0 there (asserted on the float64 reference); the kernel's sign must be 0 as well:
    nothing into the consistency sum, g_z, g_b3 or g_means from that row."""
    from da_detect_amd import _C

    C, Rb, Rc, n_src, L = 12, 0, 5, 3, 1
    for seed in range(900, 964):
        z, mask, h, w3, b3, labels, means = _ins_inputs(seed, C, Rb, Rc, n_src, L, tie=True)
        if _ins_conditions(h, w3, b3, means, Rb, Rc, n_src, True):
            break
    else:
        raise AssertionError("no seed gives a reference clear of the switching points")
    hd, wd, bd, md = (v.to(device) for v in (h, w3, b3, means))
    logits, sums = _C.da_ins_tail_forward(hd, wd, bd, None, md, Rb, Rc, n_src)
    assert float(logits[2]) == 0.0
    coef = torch.tensor([0.0, 0.9 / Rc])
    lg = logits.double().cpu()
    probe = lg.clone().requires_grad_(True)
    (0.5 - torch.sigmoid(probe[2])).abs().backward()
    assert float(probe.grad[2]) == 0.0                       # torch: d|x| / dx = 0 at x = 0
    ref = _ins_reference(z, mask, h, w3, b3, labels, means, lg, coef, Rb, Rc, n_src)
    _check("consistency sum", sums[1], *ref["consistency sum"])
    g_z, g_w3, g_b3, g_means = _C.da_ins_tail_backward(hd, wd, logits, None, md, coef.to(device), INV_KEEP, Rb, Rc, n_src)
    assert not bool(g_z[2].any())
    for name, g in (("g_z", g_z), ("g_w3", g_w3), ("g_b3", g_b3), ("g_means", g_means)):
        _check(name, g, *ref[name])
    # the other two source rows alone make g_means[0][0]: a third +-coef from the tied row would be 50 % off
    assert abs(float(ref["g_means"][0][0, 0])) in (0.0, 2 * float(coef[1].double()))


# ================================================================================= dropout rows / merge of the passes
ROWS_CASES = [(1, 1, 4), (2, 1, 4), (1, 3, 20), (2, 3, 20), (2, 2049, 1024)]     # the last: > 2048 x 256 float4 per pass


@pytest.mark.parametrize("P,R,C", ROWS_CASES, ids=lambda v: str(v))
def test_ins_dropout_rows_and_merge(device, P, R, C):
    """da_ins_dropout_rows is one fp32 multiply: bit-equal to h1 * mask.  da_ins_merge against the float64 formulas of
    include/dadet.h, g_w = [h1 > 0] sum_p m_p g_p and g_x = [h1 > 0] sum_p grl_p m_p g_p: a sum of P leaves each."""
    from da_detect_amd import _C

    g = torch.Generator().manual_seed(P * 1000 + R)
    h1 = _gated(torch.randn(R, C, generator=g))
    h1[0, 0], h1[-1, -1] = 0.0, 1.5                 # a closed and an open unit whatever the draw
    masks = torch.where(torch.rand(P, R, C, generator=g) < 0.5, INV_KEEP, 0.0).float()
    grad = torch.randn(P * R, C, generator=g)
    grl = torch.tensor([-0.1, 0.3])[:P].contiguous()
    _assert_gate_margin(h1)
    h1d, md = h1.to(device), masks.to(device)
    out = _C.da_ins_dropout_rows(h1d, md)
    assert tuple(out.shape) == (P * R, C)
    assert torch.equal(out.cpu(), (h1[None] * masks).view(P * R, C))
    g_w, g_x = _C.da_ins_merge(grad.to(device), md, h1d, grl.to(device))
    terms = masks.double() * grad.double().view(P, R, C)
    gate = (h1 > 0).double()
    _check("g_w", g_w, gate * terms.sum(0), _sum_bound(1, gate * terms.abs().sum(0), P) + FLOOR)
    wt = grl.double()[:, None, None] * terms
    _check("g_x", g_x, gate * wt.sum(0), _sum_bound(1, gate * wt.abs().sum(0), P) + FLOOR)
    closed = h1 == 0
    assert bool(closed.any()) and not bool(g_w.cpu()[closed].any()) and not bool(g_x.cpu()[closed].any())
    lean_w, lean_x = _C.da_ins_merge(grad.to(device), md, h1d, grl.to(device), need_x=False)
    assert lean_x is None and torch.equal(lean_w, g_w)


# ======================================================================================== the whole instance node once
class _GRL(torch.autograd.Function):
    """gradient scalar layer: identity forward, weight x gradient backward"""

    @staticmethod
    def forward(ctx, x, weight):
        ctx.weight = weight
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return ctx.weight * g, None


def test_instance_node_against_two_real_passes(device):
    """fused.da_instance_head (one node: stacked rows, one tail launch, one merge) at R = 12, C0 = 32, hidden widths
    64 / 64, exact-fp32 GEMMs, against float64 autograd of what the reference does: the head run TWICE on the same ROI
    features, behind GRL(-0.1) with the first pair of dropout masks for the BCE and behind GRL(+0.3) with the second pair
    for the consistency term.  Pins the stacking order, which mask belongs to which pass, and both reversal signs.
    Bar: six GEMM stages (three forward, three backward) of fp32 dot products of length K <= 64, each within (K + 2) u of
    its sum of |terms|, which for terms of random sign is about sqrt(K) = 8 times the result: 6 x 66 x 8 u = 1.9e-4 of each
    tensor's largest magnitude.  A swapped mask, row block or sign is an error of the order of the tensor itself."""
    from da_detect_amd import _C
    from da_detect_amd.modeling.da_heads import fused

    R, C0, C1, C2, L, n_src = 12, 32, 64, 64, 2, 5
    grl = torch.tensor([-0.1, 0.3])
    img = (torch.arange(R) >= n_src).long()

    def reference(p, x, means, m1, m2, labels):
        def head(xg, k):
            a1 = F.linear(xg, p["w1"], p["b1"])
            a2 = F.linear(torch.relu(a1) * m1[k], p["w2"], p["b2"])
            return a1, a2, F.linear(torch.relu(a2) * m2[k], p["w3"], p["b3"]).squeeze(1)
        a1, a2a, la = head(_GRL.apply(x, float(grl[0])), 0)
        _, a2b, lb = head(_GRL.apply(x, float(grl[1])), 1)
        bce = F.binary_cross_entropy_with_logits(la, labels)
        sg = torch.sigmoid(lb)
        cst = torch.stack([(means[l][img] - sg).abs() for l in range(L)], 1).mean()
        with torch.no_grad():
            clear = min(float(a1.abs().min()), float(a2a.abs().min()), float(a2b.abs().min()),
                        float((means[:, img] - sg[None]).abs().min()))
        return bce, cst, clear

    for seed in range(40, 168):
        g = torch.Generator().manual_seed(seed)
        p32 = {"w1": torch.randn(C1, C0, generator=g) * (3.0 / math.sqrt(C0)), "b1": torch.randn(C1, generator=g),
               "w2": torch.randn(C2, C1, generator=g) * (3.0 / math.sqrt(C1)), "b2": torch.randn(C2, generator=g),
               "w3": torch.randn(1, C2, generator=g) * (0.1 / math.sqrt(C2)), "b3": torch.tensor([0.05])}
        x32 = torch.randn(R, C0, generator=g)
        means32 = 0.15 + 0.7 * torch.rand(L, 2, generator=g)
        m1 = torch.where(torch.rand(2, R, C1, generator=g) < 0.5, INV_KEEP, 0.0).float()
        m2 = torch.where(torch.rand(2, R, C2, generator=g) < 0.5, INV_KEEP, 0.0).float()
        labels = (torch.arange(R) < n_src).float()
        p64 = {k: v.double().requires_grad_(True) for k, v in p32.items()}
        x64, means64 = x32.double().requires_grad_(True), means32.double().requires_grad_(True)
        bce_ref, cst_ref, clear = reference(p64, x64, means64, m1.double(), m2.double(), labels.double())
        if clear >= GATE:
            break
    else:
        raise AssertionError("no seed gives a reference clear of the switching points")
    assert clear >= GATE
    (0.7 * bce_ref + 1.3 * cst_ref).backward()

    head = torch.nn.Module()
    head.fc1_da, head.fc2_da, head.fc3_da = torch.nn.Linear(C0, C1), torch.nn.Linear(C1, C2), torch.nn.Linear(C2, 1)
    with torch.no_grad():
        for i, lin in enumerate((head.fc1_da, head.fc2_da, head.fc3_da), 1):
            lin.weight.copy_(p32["w%d" % i])
            lin.bias.copy_(p32["b%d" % i])
    head.to(device)
    x = x32.to(device).requires_grad_(True)
    means = means32.to(device).requires_grad_(True)
    prev = _C.get_gemm_mode()
    try:
        _C.set_gemm_mode(0)
        bce, cst, logits = fused.da_instance_head(x, head, labels.to(device), means, m1.to(device), m2.to(device),
                                                  grl.to(device), ("bce", "cst"), n_src)
        (0.7 * bce + 1.3 * cst).backward()
        torch.cuda.synchronize()
    finally:
        _C.set_gemm_mode(prev)
    assert tuple(logits.shape) == (2, R)
    pairs = [("loss bce", bce, bce_ref), ("loss cst", cst, cst_ref), ("d x", x.grad, x64.grad),
             ("d means", means.grad, means64.grad)]
    for i, lin in enumerate((head.fc1_da, head.fc2_da, head.fc3_da), 1):
        pairs += [("d w%d" % i, lin.weight.grad, p64["w%d" % i].grad), ("d b%d" % i, lin.bias.grad, p64["b%d" % i].grad)]
    for name, got, ref in pairs:
        ref = ref.detach().reshape(got.shape)
        assert float(ref.abs().max()) > 0.0, name
        _check(name, got, ref, 6 * 66 * 8 * U * float(ref.abs().max()))


# ============================================================================================================ triplet
def _triplet_inputs(seed, C, H, W):
    g = torch.Generator().manual_seed(seed)
    a, p, n = (torch.randn(1, C, H, W, generator=g) for _ in range(3))
    if C * H >= 4:                        # one (h, c) whose positive sits at a + eps: d_ap == 0 exactly, hinge active
        a[0, 0, 0, :] = 0.0
        p[0, 0, 0, :] = EPS32
        n[0, 0, 0, :] = 0.02 * torch.randn(W, generator=g)
    return a, p, n


def _triplet_reference(a, p, n, margin, g_scale):
    a64, p64, n64 = (v.double().requires_grad_(True) for v in (a, p, n))
    loss_sum = torch.nn.TripletMarginLoss(margin=margin, p=2, eps=EPS32, reduction="sum")(a64, p64, n64)
    ga, gp, gn = torch.autograd.grad(g_scale * loss_sum, (a64, p64, n64))
    with torch.no_grad():
        dp, dn = a64 - p64 + EPS32, a64 - n64 + EPS32
        dap, dan = dp.norm(dim=-1), dn.norm(dim=-1)                           # [1, C, H]
        W = a.shape[-1]
        lp, ln = a64.abs() + p64.abs() + EPS32, a64.abs() + n64.abs() + EPS32   # leaves of a - p + eps
        # d = sqrt(sum_w dp^2): the leaves' rounding (2 u each) reaches d through dp / d, a unit vector, so by
        # Cauchy-Schwarz through ||leaves||_2; W additions and the square root act on d <= ||leaves||_2
        b_dap, b_dan = (_sum_bound(W, l.norm(dim=-1)) for l in (lp, ln))
        hinge = dap - dan + margin
        active = hinge > 0
        b_loss = (_sum_bound(hinge.numel(), float(((dap + dan + margin) * active).sum()), 3)
                  + float(((b_dap + b_dan) * active).sum()))
        gs = abs(g_scale)

        def side(d, b_d, diff, leaves):      # |g / d| (rounding of the leaves and of the few operations + the error of d)
            ok = (active & (d > 0))[..., None]
            dd = torch.where(d > 0, d, torch.ones_like(d))[..., None]
            return torch.where(ok, gs / dd * (18 * U * leaves + diff.abs() * b_d[..., None] / dd), torch.zeros_like(leaves))
        bp, bn = side(dap, b_dap, dp, lp), side(dan, b_dan, dn, ln)
    return dict(loss_sum=loss_sum.detach(), b_loss=b_loss, dap=dap, dan=dan, b_dap=b_dap, b_dan=b_dan, hinge=hinge,
                active=active, ga=(ga, bp + bn + U * (gp.abs() + gn.abs()) + FLOOR), gp=(gp, bp + FLOOR),
                gn=(gn, bn + FLOOR))


@pytest.mark.parametrize("C,H,W", [(1, 1, 1), (3, 5, 7), (64, 9, 13), (100, 3, 1)], ids=lambda v: str(v))
def test_triplet_against_float64(device, C, H, W):
    """triplet_w_forward / triplet_w_backward against nn.TripletMarginLoss(margin, p=2, eps, reduction="sum") in float64 and
    its autograd.  Margin 0.25 leaves hinges on both sides of zero; the gradient of an inactive one is exactly 0.  At the
    (h, c) with p = a + eps the distance is exactly 0: float64 torch gives p no gradient there, and the kernel's guard must
    do the same, without a NaN.  Bounds: distances (W + 2 + 16) u ||leaves||_2; the hinge sum as a sum of H C values of
    three leaves plus the distances' bounds; gradients g / d x (18 u leaves + |diff| x bound(d) / d) per side."""
    from da_detect_amd import _C

    margin = 0.25
    many = C * H >= 4
    for seed in range(500 + C, 500 + C + 64):
        a, p, n = _triplet_inputs(seed, C, H, W)
        g_scale = f32(0.7 / (C * H))
        ref = _triplet_reference(a, p, n, margin, g_scale)
        both_sides = bool(ref["active"].any()) and not bool(ref["active"].all())
        if float(ref["hinge"].abs().min()) >= GATE and (both_sides or not many):
            break
    else:
        raise AssertionError("no seed gives a reference clear of the switching points")
    assert float(ref["hinge"].abs().min()) >= GATE
    if many:
        assert float(ref["dap"][0, 0, 0]) == 0.0 and bool(ref["active"][0, 0, 0])
        assert not bool(ref["gp"][0][0, 0, 0].any()) and bool(ref["ga"][0][0, 0, 0].any())      # float64 torch at d_ap = 0
    ad, pd, nd = (v.to(device).contiguous(memory_format=CL) for v in (a, p, n))
    loss, dist = _C.triplet_w_forward(ad, pd, nd, margin)
    dist = dist.view(H, C, 2)
    _check("d_ap", dist[..., 0], ref["dap"][0].t(), ref["b_dap"][0].t())
    _check("d_an", dist[..., 1], ref["dan"][0].t(), ref["b_dan"][0].t())
    if many:
        assert float(dist[0, 0, 0]) == 0.0
    _check("loss", loss, (ref["loss_sum"] / (C * H)).reshape(1), ref["b_loss"] / (C * H))
    gsd = torch.tensor([g_scale], device=device)
    got = _C.triplet_w_backward(ad, pd, nd, dist.view(H * C, 2), gsd, margin)
    for name, g in zip(("ga", "gp", "gn"), got):
        assert tuple(g.shape) == (1, C, H, W)
        _check(name, g, *ref[name])
        off = ~ref["active"][..., None].expand(1, C, H, W)
        assert not bool(g.cpu()[off].any())                   # inactive hinge: exactly zero
    if many:
        assert not bool(got[1][0, 0, 0].any())                # d_ap == 0: no gradient for p, as float64 torch
    ga2, gp2, gn2 = _C.triplet_w_backward(ad, pd, nd, dist.view(H * C, 2), gsd, margin, need=(True, False, True))
    assert gp2 is None and torch.equal(ga2, got[0]) and torch.equal(gn2, got[2])


# ================================================================================== forward sums: the same bits each run
def _five_times(fn):
    first = fn()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v).all()) for v in first)
    for _ in range(4):
        again = fn()
        for x, y in zip(first, again):
            assert torch.equal(x, y), (x.flatten()[:4].tolist(), y.flatten()[:4].tolist())
    return first


def _img_spread_inputs(device):
    g = torch.Generator().manual_seed(71)
    N, HW, C1 = 2, 35001, 4
    t = _spread((N * HW, C1), g).abs().float().to(device)
    w2 = torch.randn(C1, generator=g).to(device)
    return t, w2, torch.tensor([0.1], device=device), torch.tensor([1.0, 0.0], device=device), N, HW


def _ins_spread_inputs(device):
    g = torch.Generator().manual_seed(72)
    Rb, Rc, C = 1025, 1026, 8
    h = (_spread((Rb + Rc, C), g).abs() * (torch.rand(Rb + Rc, C, generator=g) < 0.5)).float().to(device)
    w3 = torch.randn(C, generator=g).to(device)
    labels = (torch.rand(Rb, generator=g) < 0.5).float().to(device)
    means = torch.rand(2, 2, generator=g).to(device)
    return h, w3, torch.tensor([0.05], device=device), labels, means, Rb, Rc, 500


def test_img_head_forward_sums_are_bit_stable(device):
    """(2, 35001, C1 = 4): 2048 workgroups, two trips; rows per image no multiple of the wave count"""
    from da_detect_amd import _C

    args = _img_spread_inputs(device)
    _five_times(lambda: _C.da_img_head_loss_forward(*args))


def test_ins_tail_forward_sums_are_bit_stable(device):
    from da_detect_amd import _C

    args = _ins_spread_inputs(device)
    _five_times(lambda: _C.da_ins_tail_forward(*args))


def test_triplet_forward_sum_is_bit_stable(device):
    """H C = 65536, W = 4: 256 workgroups, 1024 wavefronts.  One float atomic per wavefront made this sum depend on the
    order of arrival; wave sum, four LDS slots, per-workgroup partials and da_partials_sum_kernel add it in one order."""
    from da_detect_amd import _C

    g = torch.Generator().manual_seed(73)
    a, p, n = (_spread((1, 256, 256, 4), g).float().to(device).contiguous(memory_format=CL) for _ in range(3))
    loss, _ = _five_times(lambda: _C.triplet_w_forward(a, p, n, 0.25))
    assert float(loss) > 0.0


def test_forward_launches_share_one_scratch(device):
    """image head, instance tail, image head on one stream: the per-stream scratch of workgroup partials is rewritten by
    every launch, never carried over"""
    from da_detect_amd import _C

    img, ins = _img_spread_inputs(device), _ins_spread_inputs(device)
    alone_img = _C.da_img_head_loss_forward(*img)
    alone_ins = _C.da_ins_tail_forward(*ins)
    torch.cuda.synchronize()
    first = _C.da_img_head_loss_forward(*img)
    between = _C.da_ins_tail_forward(*ins)
    second = _C.da_img_head_loss_forward(*img)
    for got, want in ((first, alone_img), (between, alone_ins), (second, alone_img)):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
