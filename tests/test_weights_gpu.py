"""The caches of forms derived from weights against the weight epoch (da_detect_amd/weights.py) on the device, the fused
optimizer's one plan per step, and the launches of a steady training step."""
import pytest
import torch
from torch.nn import Parameter

from _bars import check, elem_bound, f32, sum_bound

pytestmark = pytest.mark.gpu
CL = torch.channels_last


def test_frozen_stem_follows_a_full_bump_and_nothing_less(device):
    """a `.data` write moves no version: `bump_weight_epoch()` is the contract for it, also for a frozen stem's padded
    weight (which ignored the epoch before)"""
    from da_detect_amd import _C
    from da_detect_amd.config import cfg
    from da_detect_amd.modeling.backbone.resnet import StemWithFixedBatchNorm

    def stem_of(state=None):
        stem = StemWithFixedBatchNorm(cfg)
        if state is not None:
            stem.load_state_dict(state)
        stem.conv1.weight.requires_grad_(False)
        return stem.to(device)

    torch.manual_seed(0)
    stem = stem_of()
    x = torch.randn(1, 3, 32, 32, device=device)
    with torch.no_grad():
        y0 = stem(x).clone()
        stem.conv1.weight.data.mul_(2)
        assert torch.equal(stem(x), y0), "without the bump the padded copy of the old weight is what the contract promises"
        _C.bump_weight_epoch(trained_only=True)      # the optimizer's bump says frozen weights did not change
        assert torch.equal(stem(x), y0)
        _C.bump_weight_epoch()
        y1 = stem(x)
        want = stem_of({k: v.cpu() for k, v in stem.state_dict().items()})(x)
    assert torch.equal(y1, want) and not torch.equal(y1, y0)


@pytest.mark.parametrize("trainable", [True, False], ids=["trainable", "frozen"])
def test_conv1x1_multi_rebuilds_its_fused_weight_when_a_source_changed(device, trainable):
    from da_detect_amd import _C
    from da_detect_amd.layers import conv as L

    gen = torch.Generator().manual_seed(3)
    ws = [Parameter(torch.randn(c, 16, 1, 1, generator=gen).to(device), requires_grad=trainable) for c in (6, 3)]
    bs = [Parameter(torch.randn(c, generator=gen).to(device), requires_grad=trainable) for c in (6, 3)]
    x = torch.randn(2, 16, 5, 7, generator=gen).to(device)
    key = tuple(id(t) for t in ws + bs)
    with torch.no_grad():
        first = [o.clone() for o in L.conv1x1_multi(x, ws, bs)]
        entry = L._FUSED_1X1[key]
        again = L.conv1x1_multi(x, ws, bs)
        assert L._FUSED_1X1[key] is entry, "the second call built the fused weight again"
        assert all(torch.equal(a, b) for a, b in zip(first, again))
        ws[0].data.add_(1)
        _C.bump_weight_epoch(trained_only=True)
        got = [o.clone() for o in L.conv1x1_multi(x, ws, bs)]
    if trainable:
        assert L._FUSED_1X1[key] is not entry
        with torch.enable_grad():
            want = L.conv1x1_multi(x, ws, bs)
        assert tuple(got[0].shape) == (2, 6, 5, 7) and tuple(got[1].shape) == (2, 3, 5, 7)
        assert all(torch.equal(a, b.detach()) for a, b in zip(got, want)) and not torch.equal(got[0], first[0])
    else:
        # the optimizer's bump says that frozen weights did not change: what derives from them alone stays
        assert L._FUSED_1X1[key] is entry and all(torch.equal(a, b) for a, b in zip(got, first))
        with torch.no_grad():
            _C.bump_weight_epoch()
            got = L.conv1x1_multi(x, ws, bs)
            assert L._FUSED_1X1[key] is not entry and not torch.equal(got[0], first[0])


def _three(device, seed):
    gen = torch.Generator().manual_seed(seed)
    ps = [Parameter(torch.randn(8, 4, 3, 3, generator=gen).to(device).contiguous(memory_format=CL)),
          Parameter(torch.randn(5, generator=gen).to(device)), Parameter(torch.randn(7, 3, generator=gen).to(device))]
    for p in ps:
        p.grad = torch.empty_like(p)
    return ps


def test_fused_sgd_builds_its_table_when_the_rows_change_and_only_then(device):
    from da_detect_amd.solver import FusedSGD

    runs = []
    for _ in range(2):
        ps = _three(device, 5)
        opt = FusedSGD([{"params": [p], "weight_decay": 1e-4 * i} for i, p in enumerate(ps)], 0.1, momentum=0.9)
        gen = torch.Generator().manual_seed(6)
        plans = []
        for lr in (0.1, 0.05, 0.025, 0.025):
            for g in opt.param_groups:
                g["lr"] = lr
            for p in ps:
                p.grad.copy_(torch.randn(p.shape, generator=gen))
            opt.step()
            plans.append(opt._plan)
        assert plans[0] is not plans[1] and plans[1] is not plans[2], "a new lr is a new table"
        assert plans[3] is plans[2], "same pointers, lr and weight decay: the table of the step before"
        assert not plans[0].by_bucket and plans[0].ranges == [(0, 3, 8 * 4 * 3 * 3)] and len(plans[0].rows) == 3
        runs.append([p.detach().clone() for p in ps] + [opt.state[p]["momentum_buffer"].clone() for p in ps])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert runs[0][3].stride() == runs[0][0].stride() and runs[0][0].is_contiguous(memory_format=CL)


class _StubReducer(object):
    """what FusedSGD asks of a reducer, for one parameter in one bucket"""
    world_size, mean_scale = 1, 1.0

    def __init__(self, p, hand_over):
        self.buckets, self.hand_over = [dict(params=[p])], hand_over

    def can_hand_over_buckets(self):
        return self.hand_over

    def update_ids(self):
        return frozenset(id(p) for p in self.buckets[0]["params"])

    def finalize(self, mean=True, per_bucket=None):
        for i, b in enumerate(self.buckets if per_bucket is not None else ()):
            per_bucket(i, b)


def test_fused_sgd_layout_rule(device):
    """the kernel walks raw storage: a gradient in another layout than its parameter is copied into it — unless it lives in
    a reducer's bucket, where replacing it would take the parameter out of the collectives: that is an error"""
    from da_detect_amd import _lib
    from da_detect_amd.solver import FusedSGD

    gen = torch.Generator().manual_seed(8)
    start = ((0.5 + torch.rand(8, 4, 3, 3, generator=gen)) * torch.where(torch.rand(8, 4, 3, 3, generator=gen) < 0.5, -1.0, 1.0))
    grads = [torch.rand(8, 4, 3, 3, generator=gen) * 2 - 1 for _ in range(2)]
    lr, wd, momentum = 0.01, 5e-4, 0.9
    p = Parameter(start.to(device).contiguous(memory_format=CL))
    opt = FusedSGD([p], lr, momentum=momentum, weight_decay=wd)
    p64 = Parameter(start.double())
    ref = torch.optim.SGD([p64], f32(lr), momentum=f32(momentum), weight_decay=f32(wd))
    bmag = torch.zeros_like(start, dtype=torch.float64)
    for g in grads:
        bmag = f32(momentum) * bmag + g.double().abs() + f32(wd) * p64.detach().abs()
        p.grad = g.to(device)                                # NCHW-contiguous: not the parameter's layout
        assert p.grad.stride() != p.stride()
        p64.grad = g.double()
        opt.step()
        ref.step()
        assert p.grad.stride() == p.stride() and torch.equal(p.grad.cpu(), g)
    assert float(p64.detach().abs().min()) >= 0.31
    check("parameter", p.detach(), p64.detach(), elem_bound(p64.detach()))
    check("momentum", opt.state[p]["momentum_buffer"], ref.state[p64]["momentum_buffer"], sum_bound(len(grads), bmag, 2))

    for hand_over in (False, True):
        q = Parameter(start.to(device).contiguous(memory_format=CL))
        other = Parameter(torch.zeros(3, device=device))
        other.grad = torch.ones(3, device=device)
        opt = FusedSGD([other, q], lr, momentum=momentum)
        opt.reducer = _StubReducer(q, hand_over)
        opt.reducer.buckets[0]["params"].append(other)
        q.grad = grad = grads[0].to(device)
        before = q.detach().clone()
        with pytest.raises(_lib.DadetError, match=r"parameter 1, shape \(8, 4, 3, 3\)"):
            opt.step()
        assert q.grad is grad and torch.equal(q.detach(), before) and float(other.detach().abs().max()) == 0.0


def test_steady_training_steps_issue_one_sequence_of_launches(device, monkeypatch):
    """five steps of the small da_plain model: from the third on every step issues the same library calls, with ONE
    optimizer launch, ONE batched transpose of the weights and ONE batched pass over their maxima.  (One
    dadet_conv_weight_transpose_padded per step is what this recipe issued before the caches shared their rule, too: a
    weight outside the transposed-weight cache.)"""
    from da_detect_amd import _lib
    from da_detect_amd.data.synthetic import make_batch
    from da_detect_amd.engine.trainer import enable_overlapped_rpn_backward, train_step
    from da_detect_amd.modeling.detector import build_detection_model
    from da_detect_amd.parallel.reducer import BucketedGradReducer
    from da_detect_amd.solver import make_optimizer
    from golden.cases import case_cfg
    from golden.fill import fill_state_dict

    c = case_cfg("da_plain")
    model = build_detection_model(c)
    model.load_state_dict(fill_state_dict(model.state_dict(), 3))
    model = model.to(device).train()
    opt = make_optimizer(c, model)
    opt.attach_reducer(BucketedGradReducer([p for p in model.parameters() if p.requires_grad], bucket_bytes=8 << 20))
    enable_overlapped_rpn_backward(model)
    images, targets = make_batch(c, 2, 192, 320, seed=100, device=device)
    names, call = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: names.append(name) or call(name, *a))
    steps = []
    for it in range(5):
        torch.manual_seed(50 + 10 * it)
        for g in opt.param_groups:                          # a per-iteration schedule: a new table every step
            g["lr"] = g["lr"] * 0.97
        del names[:]
        train_step(model, opt, images, targets)
        torch.cuda.synchronize()
        steps.append(list(names))
    assert steps[2] == steps[3] == steps[4]
    counts = {n: steps[4].count(n) for n in ("dadet_sgd_step", "dadet_conv_weight_transpose_batch", "dadet_amax_batch",
                                             "dadet_conv_weight_transpose_padded")}
    assert counts == {"dadet_sgd_step": 1, "dadet_conv_weight_transpose_batch": 1, "dadet_amax_batch": 1,
                      "dadet_conv_weight_transpose_padded": 1}, counts
