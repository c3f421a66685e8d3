"""The weight epoch and the one rule for "is this derived form still valid?" (da_detect_amd/weights.py), and the caches
that ask it, on CPU tensors with the recording stand-in for the library's `call` of tests/test_amax_host.py."""
import gc
import weakref

import torch
from torch.nn import Parameter

from da_detect_amd import amax, weights
from da_detect_amd.weights import Stamp
from test_amax_host import _held, _weight_slots_on_cpu


def _pair():
    return Parameter(torch.ones(4, 3)), Parameter(torch.ones(5), requires_grad=False)


def test_stamp_truth_table():
    w, f = _pair()
    s = Stamp.of(w, None, f)
    assert s.holds(w, None, f) and s.holds() and s.intact()
    assert s.sources()[0] is w and s.sources()[1] is None and s.sources()[2] is f
    # an absent source is part of what was recorded
    assert not s.holds(w, f, None) and not s.holds(w, torch.zeros(1), f) and not s.holds(w, None)
    assert not Stamp.of(w, f).holds(w, None)

    w, f = _pair()                                  # an ATen in-place write moves the version
    sw, sf = Stamp.of(w), Stamp.of(f)
    with torch.no_grad():
        w.mul_(2.0)
        f.mul_(2.0)
    assert not sw.holds(w) and not sf.holds(f)

    w, f = _pair()                                  # a write through .data moves nothing: the documented gap that bump() closes
    sw = Stamp.of(w)
    w.data.mul_(2.0)
    assert sw.holds(w)

    w, f = _pair()                                  # new storage under the same object and version
    sw = Stamp.of(w)
    keep = w.data                                   # (the old allocation stays: its address is not handed out again)
    w.data = torch.ones(4, 3)
    assert not sw.holds(w) and not sw.intact()
    del keep

    buf = torch.zeros(8)                            # another object at the same address, with the same version
    a, b = buf[:4], buf[:4]
    assert a.data_ptr() == b.data_ptr() and a._version == b._version
    sa = Stamp.of(a)
    assert sa.holds(a) and not sa.holds(b)
    del a
    gc.collect()
    assert not sa.holds(b) and not sa.holds() and not sa.intact() and sa.sources() == [None]


def test_stamp_follows_the_two_counters():
    w, f = _pair()
    sw, sf, both = Stamp.of(w), Stamp.of(f), Stamp.of(w, f)
    e = weights.epoch()
    weights.bump(trained_only=True)                 # the optimizer's: frozen weights did not change
    assert weights.epoch() == e + 1
    assert not sw.holds(w) and sf.holds(f) and not both.holds(w, f)
    sw.renew()
    both.renew()
    assert sw.holds(w) and both.holds(w, f)
    weights.bump()                                  # a checkpoint load, a broadcast, a manual .data write: everything
    assert weights.epoch() == e + 2
    assert not sw.holds(w) and not sf.holds(f) and not both.holds(w, f)
    sf.renew()
    assert sf.holds(f)
    sf.void()
    assert not sf.holds(f) and sf.intact(f)
    # a buffer the library rewrites behind every step is told so, whatever its requires_grad says
    t = torch.ones(3)
    st = Stamp.of(t, trained=True)
    weights.bump(trained_only=True)
    assert not st.holds(t) and Stamp.of(t).holds(t)


def test_weight_slots_measure_a_stale_frozen_entry_with_the_trained_ones(monkeypatch):
    """refresh(trained_only=True) used to mark every frozen entry current without measuring it — a frozen
    weight written through .data and followed by a bump with no device kept its old maximum for good"""
    ws, fake = _weight_slots_on_cpu(monkeypatch)
    dev = torch.device("cpu")
    f = fake.know(Parameter(torch.full((8, 4), 2.0), requires_grad=False))
    t = fake.know(Parameter(torch.full((16,), 0.5)))
    ws.ptr(f, weights.epoch()), ws.ptr(t, weights.epoch())
    assert (_held(ws, f), _held(ws, t)) == (2.0, 0.5)
    # the optimizer's step: only t changed, says the bump (f is written here to SEE that nothing measures it)
    t.data.mul_(2.0)
    f.data.mul_(3.0)
    weights.bump(trained_only=True)
    ws.refresh(dev, weights.epoch(), trained_only=True)
    assert fake.calls.count("dadet_amax_batch") == 1
    assert (_held(ws, f), _held(ws, t)) == (2.0, 1.0)       # the frozen entry was current: left alone
    n = len(fake.calls)
    ws.ptr(f, weights.epoch()), ws.ptr(t, weights.epoch())
    assert len(fake.calls) == n and _held(ws, f) == 2.0
    # the write is announced (no device: nothing launched), no GEMM asks, the optimizer steps
    weights.bump()
    t.data.mul_(2.0)
    weights.bump(trained_only=True)
    ws.refresh(dev, weights.epoch(), trained_only=True)
    assert fake.calls[n:] == ["dadet_amax_batch"]
    assert (_held(ws, f), _held(ws, t)) == (6.0, 2.0)       # measured with the trained one
    n = len(fake.calls)
    assert ws.ptr(f, weights.epoch()).value == ws.by_dev[0]["slots"].data_ptr() + 4 * ws.by_dev[0]["entries"][
        (f.data_ptr(), f.numel())]["i"]
    assert len(fake.calls) == n and _held(ws, f) == 6.0     # and current from then on
    weights.bump(trained_only=True)
    f.data.mul_(2.0)
    ws.refresh(dev, weights.epoch(), trained_only=True)
    assert _held(ws, f) == 6.0


def _transposes_on_cpu(monkeypatch):
    from da_detect_amd import _C

    ws, fake = _weight_slots_on_cpu(monkeypatch)
    monkeypatch.setattr(amax, "WEIGHTS", ws)
    monkeypatch.setattr(weights, "_stream", lambda: None)
    monkeypatch.setattr(_C, "_mode4", lambda: False)
    return weights._TransposeCache(), fake


def test_transpose_cache_refreshes_once_per_epoch_and_lets_a_model_go(monkeypatch):
    tc, fake = _transposes_on_cpu(monkeypatch)
    dev = torch.device("cpu")
    CL = torch.channels_last
    w = Parameter(torch.randn(8, 4, 3, 3).contiguous(memory_format=CL))
    w2 = Parameter(torch.randn(4, 4, 1, 1).contiguous(memory_format=CL))
    scale = torch.ones(8)
    wt = tc.get(w, scale)
    wt2 = tc.get(w2.view(4, 4, 1, 1), None)                 # a view that is gone at once: its parameter is what is held
    assert fake.calls == ["dadet_conv_weight_transpose_padded"] * 2 and tuple(wt.shape) == (4, 8, 3, 3)
    assert tc.get(w, scale) is wt and tc.get(w2.view(4, 4, 1, 1), None) is wt2 and len(fake.calls) == 2
    gc.collect()
    weights.bump(trained_only=True)                          # raw-pointer update: first request of the epoch, ONE launch
    assert tc.get(w, scale) is wt and tc.get(w2, None) is wt2 and tc.get(w, scale) is wt
    assert fake.calls[2:] == ["dadet_conv_weight_transpose_batch"] and len(tc.entries) == 2
    with torch.no_grad():
        w2.mul_(2.0)                                         # a versioned write: that entry alone
    assert tc.get(w2, None) is wt2 and fake.calls[3:] == ["dadet_conv_weight_transpose_padded"]
    assert tc.get(w2, None) is wt2 and len(fake.calls) == 4
    # the model goes away: nothing in the table keeps its weights, and the buffers go with the entries
    buf, wref = weakref.ref(wt), weakref.ref(w)
    del w, wt
    gc.collect()
    assert wref() is None and buf() is not None
    weights.bump(trained_only=True)
    tc.refresh_all(dev, sync=False)
    assert len(tc.entries) == 1 and buf() is None
    assert fake.calls[4:] == ["dadet_conv_weight_transpose_batch"]
    del scale, w2, wt2
    gc.collect()
    weights.bump(trained_only=True)
    n = len(fake.calls)
    tc.refresh_all(dev, sync=False)
    assert not tc.entries and len(fake.calls) == n           # nothing left to launch for
