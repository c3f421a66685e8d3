"""MODEL.BACKBONE.FREEZE_CONV_BODY_AT 0 and 1 on the HIP path: the max-pool backward kernel (fused with the stem's ReLU
gate and FrozenBN scale), the stem's weight gradient through the zero-padded [64,4,7,8] kernel, the stem autograd node, and
stem + res2 trained below the rest of the network.

Bars.  The pooling backward moves and adds fp32 values in ATen's order: bit-identical to ATen on the CPU.  The weight
gradient is linear in its operands: rounding level against float64 (the bound of tests/test_ops_gpu.py).  Whole-stage
gradients go through ReLUs and pooling windows whose decision can fall the other way in fp32 than in float64: the two-tier
rule of test_default_path_gpu._check_gradients."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
CL = torch.channels_last
FREEZE = "MODEL.BACKBONE.FREEZE_CONV_BODY_AT"

POOL_SHAPES = [
    # N, C, H, W
    (1, 4, 1, 1), (1, 4, 2, 3),
    (2, 8, 7, 9), (2, 8, 8, 8),       # odd / even extents: the last window is full in one and cut in the other
    (2, 64, 33, 47),
    (2, 64, 131, 259),                # 1.09 M float4 against the launch's cap of 2048 x 256 threads: a second grid-stride round
]


def _pool_backward_reference(y, gp, scale):
    """ATen on the CPU, fp32: max_pool2d(y, 3, 2, 1) backward, then * (y > 0) * scale"""
    yy = y.clone().requires_grad_(True)
    F.max_pool2d(yy, 3, 2, 1).backward(gp)
    g = yy.grad * (y > 0)
    return g if scale is None else g * scale.view(1, -1, 1, 1)


@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_maxpool_relu_backward_is_aten_bit_for_bit(device, shape):
    from da_detect_amd import _C, amax

    N, C, H, W = shape
    gen = torch.Generator().manual_seed(sum(shape))
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    gp = torch.randn((N, C, Ho, Wo), generator=gen)
    scale = torch.rand(C, generator=gen) + 0.5
    ties = torch.randint(0, 3, shape, generator=gen).float()        # non-zero ties in most windows
    smooth = F.relu(torch.randn(shape, generator=gen))
    prev = _C.get_gemm_mode()
    try:
        _C.set_gemm_mode(4)
        for y, sc in ((ties, scale), (smooth, scale), (ties, None)):
            want = _pool_backward_reference(y, gp, sc)
            g = _C.maxpool3x3s2_relu_backward(y.to(device).contiguous(memory_format=CL),
                                              gp.to(device).contiguous(memory_format=CL),
                                              sc.to(device) if sc is not None else None)
            assert g.is_contiguous(memory_format=CL) or g.numel() == g.shape[1]
            assert torch.equal(g.cpu(), want), "max |diff| %.3e" % float((g.cpu() - want).abs().max())
            # contraction mode 4: the slot that travels with g holds its largest magnitude exactly
            assert amax.value(g) == float(want.abs().max())
    finally:
        _C.set_gemm_mode(prev)


def _stem_wgrad(x4, g):
    from da_detect_amd import _C

    return _C.conv_wgrad(x4, g, (64, 4, 7, 8), stride=2, pad=3)


@pytest.mark.parametrize("mode", [4, 0])
def test_stem_weight_gradient_matches_float64(device, mode):
    """_C.conv_wgrad on the stem's geometry (stride 2, a 7 x 8 window of 4 channels: K = 224, Ho x Wo taken from the
    gradient map) against the float64 weight gradient of F.conv2d, no ReLU in between.  Bound: max |error| / mean |dW| <
    1e-4, the bound of tests/test_ops_gpu.py::test_conv_wgrad_split_bf16_modes for the default contraction mode (the
    `(4, 1e-4)` entry of its parametrize line, applied by `assert err_split < tol`)."""
    from da_detect_amd import _C

    gen = torch.Generator().manual_seed(37 * 53)
    x = torch.randn((2, 3, 37, 53), generator=gen) * 50.0
    Ho, Wo = _C.conv_out_size(37, 53, 7, 7, 2, 3)
    assert (Ho, Wo) == (19, 27)
    g = torch.randn((2, 64, Ho, Wo), generator=gen)
    w64 = torch.zeros((64, 3, 7, 7), dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w64, None, 2, 3).backward(g.double())
    prev = _C.get_gemm_mode()
    try:
        _C.set_gemm_mode(mode)
        dw4 = _stem_wgrad(_C.nchw3_to_nhwc4(x.to(device)), g.to(device).contiguous(memory_format=CL)).cpu()
    finally:
        _C.set_gemm_mode(prev)
    assert tuple(dw4.shape) == (64, 4, 7, 8)
    assert float(dw4[:, 3].abs().max()) == 0.0, "the staged input's fourth channel is zero"
    err = float((dw4[:, :3, :, :7].double() - w64.grad).abs().max()) / float(w64.grad.abs().mean())
    print("stem wgrad mode %d: max |error| / mean |dW| = %.2e" % (mode, err))
    assert err < 1e-4


def _filled_stem(device, seed=5):
    from da_detect_amd.modeling.backbone.resnet import StemWithFixedBatchNorm
    from golden.cases import case_cfg
    from golden.fill import fill_state_dict

    stem = StemWithFixedBatchNorm(case_cfg("da_plain"))
    # (keys as in the whole model, so that the fill gives the stem weight its pixel-scale standard deviation)
    sd = fill_state_dict({"stem." + k: v for k, v in stem.state_dict().items()}, seed)
    stem.load_state_dict({k[5:]: v for k, v in sd.items()})
    return stem.to(device).train()


def test_stem_node_is_the_two_pieces_chained(device, monkeypatch):
    """odd height and width: the out_size-trimmed 19 x 27 map (the 7 x 8 window alone would give 19 x 26)"""
    from da_detect_amd import _C

    stem = _filled_stem(device)
    gen = torch.Generator().manual_seed(3)
    x = (torch.randn((2, 3, 37, 53), generator=gen) * 50.0).to(device)
    stem.conv1.weight.requires_grad_(False)
    frozen = stem(x)
    assert not frozen.requires_grad
    stem.conv1.weight.requires_grad_(True)
    seen = []
    orig = _C.maxpool3x3s2
    monkeypatch.setattr(_C, "maxpool3x3s2", lambda y: seen.append(y) or orig(y))
    out = stem(x)
    monkeypatch.setattr(_C, "maxpool3x3s2", orig)
    assert out.requires_grad and torch.equal(out.detach(), frozen)
    (y,) = seen
    assert tuple(y.shape) == (2, 64, 19, 27) and tuple(out.shape) == (2, 64, 10, 14)
    gp = torch.randn(out.shape, generator=gen).to(device).contiguous(memory_format=CL)
    out.backward(gp)
    assert stem.conv1.weight.grad is not None and tuple(stem.conv1.weight.grad.shape) == (64, 3, 7, 7)
    g = _C.maxpool3x3s2_relu_backward(y, gp, stem.bn1.folded()[0])
    want = _stem_wgrad(_C.nchw3_to_nhwc4(x), g)[:, :3, :, :7]
    assert torch.equal(stem.conv1.weight.grad, want)
    assert float(want.abs().max()) > 0.0
    # no_grad / a frozen weight: today's path, no node
    with torch.no_grad():
        assert torch.equal(stem(x), frozen)


# ---- stem + res2 of the R-50-C4 body under the float64 oracle ---------------------------------------------------------
_BODY_SEED, _BODY_HW = 7, (45, 61)
_CACHE = {}


def _body_inputs():
    gen = torch.Generator().manual_seed(_BODY_SEED)
    x = torch.randn((2, 3) + _BODY_HW, generator=gen) * 50.0
    R = torch.randn((2, 256, 12, 16), generator=gen)      # 45 x 61 -> 23 x 31 (conv) -> 12 x 16 (pool)
    return x, R


def _run_body(freeze_at, device):
    """stem + layer1 of ResNet(R-50-C4) with FREEZE_CONV_BODY_AT = freeze_at, loss = sum(out * R): the gradients, and the
    number of GEMM launches (_C.conv_forward) its backward made.  One run per level, shared by the tests."""
    if freeze_at in _CACHE:
        return _CACHE[freeze_at]
    from da_detect_amd import _C
    from da_detect_amd.modeling.backbone.resnet import ResNet
    from golden.cases import case_cfg
    from golden.fill import fill_state_dict

    c = case_cfg("da_plain")
    c.merge_from_list([FREEZE, freeze_at])
    body = ResNet(c)
    sd = fill_state_dict(body.state_dict(), _BODY_SEED)
    body.load_state_dict(sd)
    body = body.to(device).train()
    assert body.layer1.input_is_relu is False
    x, R = _body_inputs()
    pooled = body.stem(x.to(device))
    out = body.layer1(pooled)
    calls = []
    orig = _C.conv_forward
    _C.conv_forward = lambda *a, **k: calls.append(1) or orig(*a, **k)
    try:
        (out * R.to(device)).sum().backward()
    finally:
        _C.conv_forward = orig
    torch.cuda.synchronize()
    res = dict(sd=sd, pooled_requires_grad=pooled.requires_grad, backward_gemms=len(calls),
               requires_grad={n: p.requires_grad for n, p in body.named_parameters()},
               grads={n: (p.grad.detach().cpu().clone() if p.grad is not None else None)
                      for n, p in body.named_parameters() if n.startswith(("stem.", "layer1."))})
    _CACHE[freeze_at] = res
    return res


def _oracle_stem_res2(sd):
    """oracle.model_ref's frozen_bn / stage and the stem lines of its backbone_c4, float64, every stem / layer1 weight
    trainable (freezing the stem changes no gradient above it): one run, shared"""
    if "oracle" in _CACHE:
        return _CACHE["oracle"]
    from oracle import model_ref

    osd = {k: (v.clone().double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    names = [k for k in osd if k.startswith(("stem.", "layer1.")) and
             k.endswith((".conv1.weight", ".conv2.weight", ".conv3.weight", ".downsample.0.weight"))]
    for n in names:
        osd[n].requires_grad_(True)
    x, R = _body_inputs()
    y = F.relu(model_ref.frozen_bn(F.conv2d(x.double(), osd["stem.conv1.weight"], None, 2, 3), osd, "stem.bn1"))
    y = F.max_pool2d(y, kernel_size=3, stride=2, padding=1)
    out = model_ref.stage(y, osd, "layer1", 3, 1)
    (out * R.double()).sum().backward()
    _CACHE["oracle"] = {n: osd[n].grad for n in names}
    return _CACHE["oracle"]


def _check_against_oracle(got, want, what):
    """test_default_path_gpu._check_gradients with its own bounds: every tensor under its flip bound (4e-3 relative L2),
    the median tensor at its rounding level (5e-5) — a ReLU or a pool argmax that falls the other way in fp32 than in
    float64 is the documented exception there, and one such unit high in res2 taints every tensor below it"""
    from test_default_path_gpu import _check_gradients

    errs = sorted((float((got[n].double() - want[n]).norm()) / (float(want[n].norm()) + 1e-30), n) for n in got)
    print("%s vs the float64 oracle, relative L2 per tensor: %s" % (what, ", ".join("%s %.2e" % (n, e) for e, n in errs)))
    for n, g in got.items():
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0.0, n
    _check_gradients(got, want, flipped_share=0.5)
    assert errs[len(errs) // 2][0] < 5e-5, "median relative L2 gradient error %.2e" % errs[len(errs) // 2][0]


def test_stem_and_res2_gradients_match_the_float64_oracle(device):
    run = _run_body(0, device)
    assert run["pooled_requires_grad"]
    trainable = [n for n in run["grads"] if run["requires_grad"][n]]
    assert "stem.conv1.weight" in trainable and len(trainable) == 11      # + 3 x 3 convs and the projection shortcut
    want = _oracle_stem_res2(run["sd"])
    assert sorted(want) == sorted(trainable)
    _check_against_oracle({n: run["grads"][n] for n in trainable}, want, "FREEZE_CONV_BODY_AT 0")


def test_freeze_at_1_trains_res2_above_a_frozen_stem(device):
    run = _run_body(1, device)
    assert not run["pooled_requires_grad"]
    stem = [n for n in run["requires_grad"] if n.startswith("stem.")]
    assert stem and all(not run["requires_grad"][n] and run["grads"][n] is None for n in stem)
    layer1 = [n for n in run["requires_grad"] if n.startswith("layer1.")]
    assert len(layer1) == 10 and all(run["requires_grad"][n] for n in layer1)
    want = _oracle_stem_res2(run["sd"])
    _check_against_oracle({n: run["grads"][n] for n in layer1}, {n: want[n] for n in layer1}, "FREEZE_CONV_BODY_AT 1")
    # no data gradient for the block's input: the two GEMMs of layer1.0 that FREEZE_CONV_BODY_AT 0 adds (through conv1 and
    # through the projection shortcut) are not launched
    assert run["backward_gemms"] == _run_body(0, device)["backward_gemms"] - 2


# ---- the whole model -------------------------------------------------------------------------------------------------
def _golden_step(freeze_at, device):
    """da_plain golden case (192 x 320), the fixture's RPN maps injected: one forward and backward"""
    from da_detect_amd.data.synthetic import make_batch
    from da_detect_amd.modeling.detector import build_detection_model
    from golden.cases import case_cfg
    from golden.fill import fill_state_dict
    from test_model_gpu import _run_with_golden_rpn_selection

    z = np.load(os.path.join(GOLD, "da_plain.npz"))
    c = case_cfg("da_plain")
    c.merge_from_list([FREEZE, freeze_at])
    model = build_detection_model(c)
    model.load_state_dict(fill_state_dict(model.state_dict(), int(z["seed"])))
    model = model.to(device).train()
    seed, H, W, nimg = int(z["seed"]), int(z["H"]), int(z["W"]), int(z["nimg"])
    images, targets = make_batch(c, nimg, H, W, seed=seed, device=device)
    losses, _ = _run_with_golden_rpn_selection(model, z, images, targets, seed, device, inject=True)
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    return c, model, images, {k: v.detach().cpu() for k, v in losses.items()}


def _frozen_and_unfrozen(device):
    """the golden step at FREEZE_CONV_BODY_AT 2 and 0 from one state dict: one run each, shared"""
    if "pair" not in _CACHE:
        _, frozen, _, losses2 = _golden_step(2, device)
        c, model, images, losses0 = _golden_step(0, device)
        _CACHE["pair"] = (c, frozen, model, images, losses2, losses0)
    return _CACHE["pair"]


# parameters whose gradient da_img_bwd_kernel / da_ins_bwd_n_kernel (csrc/da_heads.hip) sum with float atomics
_ATOMIC_GRADS = ("da_heads.imghead.conv2_da.weight", "da_heads.imghead.conv2_da.bias",
                 "da_heads.inshead.fc3_da.weight", "da_heads.inshead.fc3_da.bias")


def test_unfreezing_changes_no_loss(device):
    """FREEZE_CONV_BODY_AT 2 against 0 from one state dict: the loss dicts are bit-identical.  (The three DA losses are
    part of this since da_img_fwd_kernel and da_ins_fwd_n_kernel add their partial sums in a fixed order: with float atomics
    they differed in the last bits between two runs of ONE model — 1.03337121 / 1.03337097, 1.26122475 / 1.26122487,
    0.340123802 / 0.340123713 at level 2 — and so between the levels.)"""
    _, _, _, _, losses2, losses0 = _frozen_and_unfrozen(device)
    assert set(losses0) == set(losses2)
    for k in losses2:
        print("%-20s level 2 %.9g  level 0 %.9g" % (k, float(losses2[k]), float(losses0[k])))
    differ = [k for k in losses2 if not torch.equal(losses0[k], losses2[k])]
    assert not differ, {k: (float(losses2[k]), float(losses0[k])) for k in differ}


def test_unfreezing_adds_gradients_and_changes_none(device):
    """FREEZE_CONV_BODY_AT 2 against 0 from one state dict: every gradient both models compute is bit-identical (the same
    launches on the same operands; the second model only adds launches), stem and res2 gain finite non-zero gradients, and
    one FusedSGD step moves stem.conv1.weight by torch.optim.SGD's rule.

    Four tensors are not bit-identical, between the levels as between two runs of one level (measured: 6e-8 .. 1.7e-7
    relative L2 in both pairings): the last layers of the two DA heads, whose gradients da_img_bwd_kernel and
    da_ins_bwd_n_kernel (csrc/da_heads.hip) add with float atomics in arrival order.  They are held to 1e-6 relative L2.
    The loss dicts: test_unfreezing_changes_no_loss."""
    from da_detect_amd.solver import make_optimizer

    c, frozen, model, images, losses2, losses0 = _frozen_and_unfrozen(device)
    g2 = {n: p.grad for n, p in frozen.named_parameters() if p.requires_grad}
    g0 = {n: p.grad for n, p in model.named_parameters() if p.requires_grad}
    assert set(g2) < set(g0)
    for n, g in g2.items():
        assert g is not None and g0[n] is not None, n
        if n in _ATOMIC_GRADS:
            rel = float((g.double() - g0[n].double()).norm()) / float(g.double().norm())
            print("%s: relative L2 between the levels %.2e" % (n, rel))
            assert rel <= 1e-6, (n, rel)
        else:
            assert torch.equal(g, g0[n]), n
    low = [n for n in g0 if n.startswith(("backbone.body.stem.", "backbone.body.layer1."))]
    assert sorted(low) == sorted(set(g0) - set(g2)) and len(low) == 11
    for n in low:
        assert g0[n] is not None and bool(torch.isfinite(g0[n]).all()) and float(g0[n].abs().max()) > 0.0, n
    for n, p in frozen.named_parameters():
        if n.startswith(("backbone.body.stem.", "backbone.body.layer1.")):
            assert not p.requires_grad and p.grad is None, n

    stem = model.backbone.body.stem
    w = stem.conv1.weight
    w_before, grad = w.detach().cpu().clone(), w.grad.detach().cpu().clone()
    with torch.no_grad():
        stem(images.tensors)                      # the frozen-path cache of the padded weight now holds the old values
    opt = make_optimizer(c, model)
    opt.step()
    torch.cuda.synchronize()
    ref = torch.nn.Parameter(w_before.clone())
    ref.grad = grad.clone()
    torch.optim.SGD([ref], lr=c.SOLVER.BASE_LR, momentum=c.SOLVER.MOMENTUM, weight_decay=c.SOLVER.WEIGHT_DECAY).step()
    assert not torch.equal(w.detach().cpu(), w_before), "stem.conv1.weight did not move"
    torch.testing.assert_close(w.detach().cpu(), ref.detach(), rtol=1e-6, atol=1e-7)
    # the optimizer writes through raw pointers: the no_grad path must see the new weight as the training path does
    with torch.no_grad():
        evaluated = stem(images.tensors)
    assert torch.equal(evaluated, stem(images.tensors).detach())
