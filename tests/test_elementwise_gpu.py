"""The elementwise tail of csrc/elementwise.hip called directly through its `_C` wrappers (the SGD kernel through FusedSGD,
as tests/test_model_gpu.py::test_fused_sgd_matches_torch_sgd does), against float64 torch on the CPU, past the points where
the launches change shape: colsum's 16 / 32 / 64-column block layouts, `cols < ld`, `accumulate`, its 1024-split cap and
the empty case; the 2048-workgroup x 256-lane grid cap of the streaming kernels (524 288 items: the second trip of their
grid-stride loops); the SGD kernel's 512-workgroup cap, its scalar path and its `n % 4` tail; 3000 ground-truth boxes in
the anchor labelling's LDS table.

Bars (tests/_bars.py), u = 2^-24:  16 u |ref| + one denormal step for a value that is one chain of operations;
(n + k + 1 + 16) u S for a sum of n values of k leaves each, S over the reference's leaf magnitudes.  Copies, gates and
max pooling are exact.

SGD.  torch.optim.SGD in float64 (d = g + wd p; b = momentum b + d; p -= lr b, from b = 0), with lr, weight decay and
momentum rounded to fp32 as the kernel receives them, four steps.  Parameters start at 0.5 <= |p| < 1.5, gradients lie in
[-1, 1), lr <= 0.02, momentum 0.9: |b| <= 1.001 x (1 + 0.9 + 0.81 + 0.729) < 3.45, four steps move a parameter by less than
0.02 x (1 + 1.9 + 2.71 + 3.44) = 0.19, so |p| >= 0.31 throughout and p - lr b never cancels.  The error of b grows per step by
the roundings of wd p, of g + wd p, of momentum b and of their sum, u (0.001 + 1.001 + 3.1 + 3.45) < 7.6 u, and carries over
with weight momentum: at most 7.6 u x 3.44 = 26 u after any of the four steps.  One step's error in p is then u |p'| from
the subtraction, u lr |b| <= 0.07 u <= 0.23 u |p'| from the product and lr x 26 u = 0.52 u <= 1.7 u |p'| from b: less than
3 u |p'|, so 12 u |p| after four steps, inside the 16 u of the one-chain bar.  The momentum buffer can cancel (gradients of
random sign), so it is held to the leaf-sum bar with n = 4 steps, k = 2 leaves (g and wd p),
S = sum_j momentum^(4 - j) (|g_j| + wd |p_j|).
The kernel's `first_step` flag is never 1 from Python: FusedSGD zero-fills a new momentum buffer and passes 0, which gives
torch's first-step rule.  test_sgd_step_first_step_flag passes 1 to the library itself, over buffers filled with NaN.
The reducer's flat bucket cannot hand the kernel a slice that is not 16-byte aligned (every slot starts at a multiple of
four floats of a 256-byte aligned allocation), and momentum buffers are allocations of their own; a PARAMETER that is a
view at an odd storage offset can, and the kernel then takes the scalar path for that tensor: two such parameters here.

Every check prints its largest err / bound ratio."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from _bars import FLOOR, U, check, elem_bound, f32, spread, sum_bound

pytestmark = pytest.mark.gpu
CL = torch.channels_last
GATE = 1e-3
GRID_CAP = 2048 * 256                    # items one trip of a streaming kernel's grid covers


def _gate_input(shape, g):
    """exactly 0 (closed: the gate is y > 0), or at least 1e-3 away from 0 on either side"""
    z = torch.randn(shape, generator=g)
    y = torch.where(z > 0, z.abs() + GATE, -(z.abs() + GATE))
    y = torch.where(torch.rand(shape, generator=g) < 0.2, torch.zeros(()), y).float()
    y.view(-1)[:3] = torch.tensor([0.0, 1.5, -1.5])          # all three kinds whatever the draw
    return y


# ============================================================================================================= colsum
def _colsum_check(name, device, g, out=None, accumulate=False, cols=None, prefill=None):
    from da_detect_amd import _C

    rows, ld = g.shape
    C = ld if cols is None else cols
    g64 = g.double()[:, :C]
    want, mag, n = g64.sum(0), g64.abs().sum(0), rows
    if accumulate:
        want, mag, n = want + prefill.double(), mag + prefill.double().abs(), rows + 1
    gd = g.to(device)
    results = []
    for _ in range(3):
        o = prefill.clone().to(device) if prefill is not None else None
        results.append(_C.colsum(gd, out=o, accumulate=accumulate, cols=cols))
        if o is not None:
            assert results[-1] is o
    assert torch.equal(results[0], results[1]) and torch.equal(results[0], results[2])       # a fixed order of summation
    assert tuple(results[0].shape) == (C,)
    check(name, results[0], want, sum_bound(n, mag))


@pytest.mark.parametrize("C", [1, 16, 17, 20, 32, 33, 64, 65, 256], ids=lambda v: "C%d" % v)
def test_colsum_block_layouts(device, C):
    """16-, 32- and 64-column blocks with the last block partly idle; 1, 63, 64, 65 rows (one split, with idle row lanes)
    and 1000 rows (16 splits of 63 rows)"""
    for rows in (1, 63, 64, 65, 1000):
        g = spread((rows, C), torch.Generator().manual_seed(C * 7 + rows)).float()
        _colsum_check("colsum %d x %d" % (rows, C), device, g)


def test_colsum_split_cap_ld_accumulate_and_empty(device):
    from da_detect_amd import _C

    gen = torch.Generator().manual_seed(3)
    # 70 000 rows x 20 columns: ceil(70 000 / 64) = 1094 splits wanted, capped at 1024 (69 rows each, the last one shorter);
    # the final kernel's 64 lanes walk them in 16 trips
    _colsum_check("colsum 70000 x 20", device, spread((70000, 20), gen).float())
    for rows in (65, 1000):
        for cols, ld in ((18, 20), (27, 28)):
            g = spread((rows, ld), gen).float()
            _colsum_check("colsum %d x %d of %d" % (rows, cols, ld), device, g, cols=cols)
            _colsum_check("colsum %d x %d of %d, accumulate" % (rows, cols, ld), device, g, cols=cols, accumulate=True,
                          prefill=spread((cols,), gen).float())
        g = spread((rows, 33), gen).float()
        _colsum_check("colsum %d x 33, accumulate" % rows, device, g, accumulate=True, prefill=spread((33,), gen).float())
    # no rows: zeros, or the prefilled buffer as it was
    empty = torch.empty((0, 20), device=device)
    assert torch.equal(_C.colsum(empty), torch.zeros(20, device=device))
    assert torch.equal(_C.colsum(empty, cols=18), torch.zeros(18, device=device))
    fill = spread((20,), gen).float().to(device)
    out = fill.clone()
    assert _C.colsum(empty, out=out, accumulate=True) is out and torch.equal(out, fill)
    assert torch.equal(_C.colsum(empty, out=out, accumulate=False), torch.zeros(20, device=device))


# =================================================================================================== relu_bn_backward
RELU_BN_SHAPES = [(5, 4), (37, 20), (2, 4, 3, 5), (3, 64, 9, 11), (8200, 256)]      # the last: 524 800 float4 > the grid cap


@pytest.mark.parametrize("shape", RELU_BN_SHAPES, ids=lambda v: "x".join(str(d) for d in v))
def test_relu_bn_backward_every_form(device, shape):
    """with and without y, scale and the unscaled output: the gated copy is exact (closed where y <= 0, y == 0 included), the
    scaled one is one multiply"""
    from da_detect_amd import _C

    gen = torch.Generator().manual_seed(sum(shape))
    C = shape[1]
    assert shape[0] * C // 4 > GRID_CAP or len(shape) == 4 or shape[0] < 100
    g = torch.randn(shape, generator=gen)
    y = _gate_input(shape, gen)
    nz = y[y != 0]
    assert float(nz.abs().min()) >= GATE and bool((y == 0).any()) and bool((y < 0).any()) and bool((y > 0).any())
    scale = (0.5 + 1.5 * torch.rand(C, generator=gen)).float()
    bshape = (1, C) + (1,) * (len(shape) - 2)
    gd, yd, sd = g.to(device), y.to(device), scale.to(device)
    for with_y in (True, False):
        masked = g * (y > 0) if with_y else g
        for with_scale in (True, False):
            want = masked.double() * scale.double().view(bshape) if with_scale else masked.double()
            for want_unscaled in (True, False):
                g_out, g_scaled = _C.relu_bn_backward(gd, yd if with_y else None, sd if with_scale else None, want_unscaled)
                tag = "y=%d scale=%d unscaled=%d" % (with_y, with_scale, want_unscaled)
                if want_unscaled:
                    assert torch.equal(g_out.cpu(), masked), tag
                else:
                    assert g_out is None
                if with_scale:
                    check("g_scaled " + tag, g_scaled, want, elem_bound(want))
                    assert not bool(g_scaled.cpu()[masked == 0].any())
                else:
                    assert torch.equal(g_scaled.cpu(), masked), tag


# ============================================================================== affine, pools, staging past the grid cap
@pytest.mark.parametrize("shape", [(1, 4, 1, 1), (2, 4, 3, 5), (2, 20, 2, 3), (2, 4, 513, 512)],
                         ids=lambda v: "x".join(str(d) for d in v))
@pytest.mark.parametrize("relu", [False, True], ids=["affine", "affine+relu"])
def test_channel_affine(device, shape, relu):
    from da_detect_amd import _C

    gen = torch.Generator().manual_seed(sum(shape))
    N, C, H, W = shape
    assert N * H * W * C // 4 > GRID_CAP or N * H * W < 100
    x = torch.randn(shape, generator=gen)
    scale = (torch.randn(C, generator=gen) * 2).float()
    bias = torch.randn(C, generator=gen)
    got = _C.channel_affine(x.to(device), scale.to(device), bias.to(device), relu=relu)
    s64, b64 = scale.double().view(1, C, 1, 1), bias.double().view(1, C, 1, 1)
    want = x.double() * s64 + b64
    bound = sum_bound(1, (x.double() * s64).abs() + b64.abs(), 2) + FLOOR
    check("channel_affine", got, torch.relu(want) if relu else want, bound)         # |relu(a) - relu(b)| <= |a - b|
    if relu:
        assert float(got.min()) >= 0.0


@pytest.mark.parametrize("shape", [(3, 4, 1, 1), (3, 4, 7, 7), (2, 20, 7, 7), (8200, 256, 1, 1), (2100, 1000, 1, 2)],
                         ids=lambda v: "x".join(str(d) for d in v))
def test_avgpool_forward(device, shape):
    """a sum of HW values, then one division.  8200 x 256 and 2100 x 1000: 524 800 / 525 000 float4 outputs, past the cap"""
    from da_detect_amd import _C

    R, C, h, w = shape
    assert R * C // 4 > GRID_CAP or R < 100
    x = spread(shape, torch.Generator().manual_seed(sum(shape))).float()
    got = _C.avgpool_forward(x.to(device))
    assert tuple(got.shape) == (R, C)
    x64 = x.double()
    check("avgpool_forward", got, x64.mean((2, 3)), sum_bound(h * w, x64.abs().sum((2, 3)) / (h * w)))


@pytest.mark.parametrize("R,C,h,w", [(3, 4, 1, 1), (3, 4, 7, 7), (2, 20, 7, 7), (170, 256, 7, 7)], ids=lambda v: str(v))
def test_avgpool_backward(device, R, C, h, w):
    """170 x 49 x 64 = 533 120 float4 outputs, past the cap"""
    from da_detect_amd import _C

    assert R * h * w * C // 4 > GRID_CAP or R < 100
    gy = spread((R, C), torch.Generator().manual_seed(R + C + h)).float()
    got = _C.avgpool_backward(gy.to(device), h, w)
    assert tuple(got.shape) == (R, C, h, w)
    want = (gy.double() / (h * w)).view(R, C, 1, 1).expand(R, C, h, w)
    check("avgpool_backward", got, want, elem_bound(want))


@pytest.mark.parametrize("N,H,W", [(1, 1, 1), (2, 2, 7), (3, 8, 1), (2, 513, 512)], ids=lambda v: str(v))
def test_nchw3_to_nhwc4_is_a_copy(device, N, H, W):
    from da_detect_amd import _C

    assert N * H * W > GRID_CAP or N * H * W < 100
    x = torch.randn(N, 3, H, W, generator=torch.Generator().manual_seed(N + H + W))
    got = _C.nchw3_to_nhwc4(x.to(device))
    assert tuple(got.shape) == (N, 4, H, W) and got.is_contiguous(memory_format=CL)
    got = got.cpu()
    assert torch.equal(got[:, :3], x) and not bool(got[:, 3].any())


def test_maxpool3x3s2_is_exact(device):
    """C = 4 with H, W in {1, 2, 7, 8}: windows cut by every border, odd and even sizes; then 2 x 4 x 1026 x 1028:
    2 x 513 x 514 = 527 364 float4 outputs, past the cap"""
    from da_detect_amd import _C

    gen = torch.Generator().manual_seed(11)
    shapes = [(2, 4, H, W) for H in (1, 2, 7, 8) for W in (1, 2, 7, 8)] + [(1, 12, 7, 8), (2, 4, 1026, 1028)]
    assert 2 * 513 * 514 > GRID_CAP
    for shape in shapes:
        x = torch.randn(shape, generator=gen)
        got = _C.maxpool3x3s2(x.to(device))
        want = F.max_pool2d(x, 3, 2, 1)
        assert got.shape == want.shape and torch.equal(got.cpu(), want), shape


# ================================================================================================================ SGD
def test_fused_sgd_against_float64(device):
    from da_detect_amd.parallel.reducer import BucketedGradReducer
    from da_detect_amd.solver import FusedSGD

    gen = torch.Generator().manual_seed(0)
    # 3 000 001 = 750 000 float4 + 1: more than 512 workgroups x 1024 float4, so the stride loop runs a second trip and
    # the tail is one element; 1024 * 1024 + 3: a vector body of 256 workgroups and a tail of 3
    sizes = [1, 3, 4, 5, 1023, 1024 * 1024 + 3, 3000001, 5, 1023, 7]
    unaligned, no_grad = (7, 8), 9

    def start(n):
        return ((0.5 + torch.rand(n, generator=gen)) * torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)).float()

    init = [start(n) for n in sizes]
    ps, keep = [], []
    for i, v in enumerate(init):
        if i in unaligned:
            base = torch.zeros(v.numel() + 8, device=device)
            base[1:1 + v.numel()] = v.to(device)
            keep.append(base)
            p = torch.nn.Parameter(base[1:1 + v.numel()])
            assert p.data_ptr() % 16 == 4
        else:
            p = torch.nn.Parameter(v.to(device))
            assert p.data_ptr() % 16 == 0
        ps.append(p)
    lrs = [0.01 * (1 + i % 2) for i in range(len(sizes))]
    wds = [5e-4 * (i % 3 != 0) for i in range(len(sizes))]
    momentum = 0.9
    fused = FusedSGD([{"params": [p], "lr": lr, "weight_decay": wd} for p, lr, wd in zip(ps, lrs, wds)], 0.01,
                     momentum=momentum)
    fused.attach_reducer(BucketedGradReducer(ps, bucket_bytes=4096))
    p64 = [v.double() for v in init]
    b64 = [torch.zeros_like(v) for v in p64]
    bmag = [torch.zeros_like(v) for v in p64]
    m32 = f32(momentum)
    for step in range(4):
        fused.zero_grad()
        for i, p in enumerate(ps):
            if i == no_grad:
                continue
            g = (torch.rand(sizes[i], generator=gen) * 2 - 1).float()
            (p * g.to(device)).sum().backward()
            lr, wd = f32(lrs[i]), f32(wds[i])
            bmag[i] = m32 * bmag[i] + g.double().abs() + wd * p64[i].abs()
            b64[i] = m32 * b64[i] + g.double() + wd * p64[i]
            p64[i] = p64[i] - lr * b64[i]
            assert float(p64[i].abs().min()) >= 0.31
        fused.step()
    torch.cuda.synchronize()
    for i, p in enumerate(ps):
        if i == no_grad:
            assert torch.equal(p.detach().cpu(), init[i]) and "momentum_buffer" not in fused.state[p]
            continue
        tag = "n = %d%s" % (sizes[i], ", scalar path" if i in unaligned else "")
        check("parameter, " + tag, p.detach(), p64[i], elem_bound(p64[i]))
        check("momentum, " + tag, fused.state[p]["momentum_buffer"], b64[i], sum_bound(4, bmag[i], 2))
    for base, i in zip(keep, unaligned):             # the scalar path wrote nothing around its slice
        assert float(base[0]) == 0.0 and not bool(base[1 + sizes[i]:].any())


@pytest.mark.parametrize("offset", [0, 1], ids=["float4 path", "scalar path"])
def test_sgd_step_first_step_flag(device, offset):
    """dadet_sgd_step itself with first_step = 1: b = d without reading the buffer (NaN-filled here), grad_scale 0.5"""
    from da_detect_amd import _lib

    gen = torch.Generator().manual_seed(21 + offset)
    sizes = [1029, 6, 2]
    lr, wd, gs = f32(0.02), f32(5e-4), 0.5
    arr = (_lib.SgdEntry * len(sizes))()
    tensors = []
    for i, n in enumerate(sizes):
        p0, g0 = torch.rand(n, generator=gen) + 2.0, torch.rand(n, generator=gen) * 2 - 1
        pd = torch.zeros(n + 8, device=device)
        pd[offset:offset + n] = p0.to(device)
        gd, bd = g0.to(device), torch.full((n,), float("nan"), device=device)
        tensors.append((p0, g0, pd, gd, bd))
        arr[i].p, arr[i].g, arr[i].buf, arr[i].numel = pd.data_ptr() + 4 * offset, gd.data_ptr(), bd.data_ptr(), n
        arr[i].lr, arr[i].weight_decay = lr, wd
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)
    _lib.call("dadet_sgd_step", ctypes.c_void_p(table.data_ptr()), len(sizes), ctypes.c_int64(max(sizes)), 0.9, 1, gs,
              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for (p0, g0, pd, gd, bd), n in zip(tensors, sizes):
        d = g0.double() * gs + wd * p0.double()
        check("first step: momentum, n = %d" % n, bd, d, sum_bound(1, (g0.double() * gs).abs() + wd * p0.double().abs(), 2))
        want = p0.double() - lr * d
        check("first step: parameter, n = %d" % n, pd[offset:offset + n], want, elem_bound(want))
        assert not bool(pd[:offset].any()) and not bool(pd[offset + n:].any())


# ================================================================================================= rpn_anchor_targets
def _int_boxes(gen, n, lo, hi, min_side, max_side):
    """boxes with integer corners: every difference, area and centre is exact in fp32, so an IoU is one rounded division on
    the GPU and in the CPU chain alike"""
    xy = torch.randint(lo, hi, (n, 2), generator=gen)
    wh = torch.randint(min_side, max_side, (n, 2), generator=gen)
    return torch.cat([xy, xy + wh], 1).float()


def _anchor_chain(anchors, vis, gts, high, low):
    """the CPU chain of oracle/model_ref.py, as tests/test_ops_gpu.py::test_rpn_anchor_targets_match_the_aten_chain uses it;
    the regression targets from the same `encode` in float64 (bound: the quotient (gcx - ecx) / ew is one rounding of exact
    operands; log(gw / ew) sees the quotient's rounding as an absolute u, plus logf)"""
    from oracle import model_ref as M

    iou = M.box_iou(gts, anchors)
    m = M.matcher(iou, high, low, True)
    want = (m >= 0).float()
    want[m == M.BELOW_LOW] = 0
    want[~vis] = -1
    want[m == M.BETWEEN] = -1
    reg = M.encode(gts.double()[m.clamp(min=0)], anchors.double(), (1.0, 1.0, 1.0, 1.0))
    return iou, m, want, reg, elem_bound(reg) + 2 * U


def test_rpn_anchor_targets_box_that_no_anchor_overlaps(device):
    """a ground-truth box far from every anchor has best IoU 0, and every anchor's IoU with it EQUALS that best: the
    reference's low-quality rule (matcher.py: iou == best) then marks every anchor, whatever its own best IoU, and each
    keeps its argmax — the labels are 1 wherever the anchor is visible"""
    from da_detect_amd import _C

    gen = torch.Generator().manual_seed(5)
    anchors = _int_boxes(gen, 1500, -20, 300, 8, 120)
    gts = _int_boxes(gen, 6, 0, 300, 20, 150)
    gts[3] = torch.tensor([5000.0, 5000.0, 5060.0, 5040.0])
    anchors[7] = gts[1]
    vis = (anchors[:, 0] >= 0) & (anchors[:, 1] >= 0)
    iou, m, want, reg, b_reg = _anchor_chain(anchors, vis, gts, 0.7, 0.3)
    assert float(iou[3].max()) == 0.0 and float(iou[[0, 1, 2, 4, 5]].max(1).values.min()) > 0.0
    assert bool((m >= 0).all()) and bool((want[vis] == 1).all()) and bool((iou.max(0).values < 0.3).any())
    assert bool((~vis).any())
    lab, got = _C.rpn_anchor_targets(anchors.to(device), vis.to(device), gts.to(device), 0.7, 0.3)
    assert torch.equal(lab.cpu(), want)
    check("regression targets", got, reg, b_reg)
    # the same boxes without the far one: the usual mixture of 1 / 0 / -1
    near = gts[[0, 1, 2, 4, 5]]
    iou, m, want, reg, b_reg = _anchor_chain(anchors, vis, near, 0.7, 0.3)
    assert all(bool((want == v).any()) for v in (1.0, 0.0, -1.0)) and bool((m == -2).any())
    lab, got = _C.rpn_anchor_targets(anchors.to(device), vis.to(device), near.to(device), 0.7, 0.3)
    assert torch.equal(lab.cpu(), want)
    check("regression targets", got, reg, b_reg)


def test_rpn_anchor_targets_3000_ground_truth_boxes(device):
    """the entry point's own cap: 3000 boxes x 24 B = 72 000 B of dynamic LDS per workgroup, 256 anchors"""
    from da_detect_amd import _C

    gen = torch.Generator().manual_seed(6)
    anchors = _int_boxes(gen, 256, 0, 900, 8, 200)
    gts = _int_boxes(gen, 3000, 0, 900, 8, 200)
    anchors[5] = gts[2999]                                   # an exact match with the table's last slot
    anchors[0] = torch.tensor([0.0, 0.0, 1100.0, 1100.0])    # overlaps every box: no best IoU of 0 in this case
    vis = torch.ones(256, dtype=torch.bool)
    vis[::7] = False
    iou, m, want, reg, b_reg = _anchor_chain(anchors, vis, gts, 0.7, 0.3)
    assert float(iou.max(1).values.min()) > 0.0 and int(m[5]) >= 0
    lab, got = _C.rpn_anchor_targets(anchors.to(device), vis.to(device), gts.to(device), 0.7, 0.3)
    assert torch.equal(lab.cpu(), want)
    check("regression targets", got, reg, b_reg)
