"""The weight epoch, the one rule for "is this form derived from weights still valid?" (Stamp), and the transposed weights
of the data-gradient GEMMs.  The fused optimizer writes parameters through raw pointers, a broadcast or a checkpoint load
through `.data`: torch's version counter sees neither, so such a write is followed by `bump()`, and every cached copy,
transposed or padded form or maximum of a weight asks its Stamp ("Forms derived from weights")."""
import ctypes
import weakref

import torch

from . import _lib

_every = 0     # moves on every bump
_full = 0      # moves on a full bump only (trained_only=False: any weight may have changed, frozen ones included)


def epoch():
    """counts the in-place weight updates made through raw pointers or `.data` (see bump)"""
    return _every


class Stamp(object):
    """What a derived form was computed from.  `holds(*tensors)`: every source is the same object (held weakly; None for
    an absent one), has the same autograd version, the same address and the same extent of storage behind it (`p.data =
    ...`, .to() and re-flattening replace those under a living object and version), and sees its bump counter unmoved — a
    source with requires_grad watches every bump, a frozen one the full bumps only."""

    __slots__ = ("marks", "every", "full", "trained", "frozen")

    @classmethod
    def of(cls, *tensors, epoch=None, trained=None):
        """epoch: the every-bump counter as the caller read it (default: now).  trained=True: the sources change with every
        bump whatever their requires_grad says (a buffer this library rewrites behind the optimizer)"""
        s = cls()
        s.marks = [t if t is None else (weakref.ref(t), t._version, t.data_ptr(), t.untyped_storage().nbytes())
                   for t in tensors]
        flags = [t.requires_grad if trained is None else trained for t in tensors if t is not None]
        s.trained, s.frozen = any(flags), not all(flags)
        s.every, s.full = (_every if epoch is None else epoch), _full
        return s

    def holds(self, *tensors, epoch=None, counters=True):
        """without tensors: of the recorded objects themselves (false once one of them is gone)"""
        if counters and ((self.trained and self.every != (_every if epoch is None else epoch))
                         or (self.frozen and self.full != _full)):
            return False
        marks = self.marks
        if len(tensors) != len(marks):
            if tensors:
                return False
            tensors = self.sources()
        for m, t in zip(marks, tensors):
            if m is None or t is None:
                if m is not t:
                    return False
            elif m[0]() is not t or t._version != m[1] or t.data_ptr() != m[2] or t.untyped_storage().nbytes() != m[3]:
                return False
        return True

    def intact(self, *tensors):
        """everything but the counters"""
        return self.holds(*tensors, counters=False)

    def sources(self):
        """the recorded objects (None: absent, or gone)"""
        return [m and m[0]() for m in self.marks]

    def renew(self, epoch=None):
        """the form was just recomputed from sources that are intact: current again"""
        self.every, self.full = (_every if epoch is None else epoch), _full

    def void(self):
        """the form was overwritten: nothing holds until it is recomputed"""
        self.every = self.full = -1


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def transpose_now(w, scale, wt):
    Cout, Cin, KH, KW = w.shape
    # wt.shape[1], the rows of the result: >= Cout (zero columns behind the weight's own)
    _lib.call("dadet_conv_weight_transpose_padded", _p(w), _p(scale), _p(wt), Cout, KH, KW, Cin, wt.shape[1], _stream())
    return wt


class _TransposeCache(object):
    """Transposed (tap-flipped, FrozenBN-folded) weights for the data-gradient GEMMs, refreshed for ALL registered weights
    by ONE launch per optimizer step instead of one launch in front of every data-gradient GEMM.

    An entry (weight address, shape, scale address) owns a persistent output buffer and a Stamp of the weight and the
    scale, which it holds weakly: an entry whose source is gone, was written through ATen or moved is dropped at the next
    batched refresh, and so is one nobody asked for during the last two epochs.  The first request of an epoch recomputes
    every entry in one batched launch on the current stream; a weight seen for the first time is transposed on the spot
    and joins the table."""

    def __init__(self):
        self.entries = {}
        self.batched_epoch = -1
        self.table = None          # (device tensor, n, total_blocks, keys)
        self.ready = None          # (stream, event) of the last batched refresh

    def _single(self, e, w, scale, owners):
        """one entry on the current stream, remembered with an event for readers on other streams"""
        from . import amax
        transpose_now(w, scale, e["wt"])
        amax.WEIGHTS.invalidate(e["wt"])
        e["stamp"] = Stamp.of(*owners)
        if w.is_cuda:
            st = torch.cuda.current_stream(w.device)
            e["ev"] = (st, st.record_event())
        return e["wt"]

    def get(self, w, scale, cout_pad=0):
        Cout, Cin, KH, KW = w.shape
        key = (w.data_ptr(), Cout, Cin, KH, KW, scale.data_ptr() if scale is not None else 0, w.device.index, cout_pad)
        # what lives as long as the storage does: the parameter itself for a (short-lived) view of one
        owners = (w if w._base is None else w._base, scale if scale is None or scale._base is None else scale._base)
        e = self.entries.get(key)
        if e is None:
            wt = torch.empty((Cin, max(Cout, cout_pad), KH, KW), dtype=torch.float32, device=w.device,
                             memory_format=torch.channels_last)
            wt._dadet_persistent = True    # its largest magnitude lives in amax.WEIGHTS (mode 4)
            e = dict(wt=wt, used=_every, ev=None)
            self._single(e, w, scale, owners)
            self.entries[key] = e
            self.table = None
            return wt
        e["used"] = _every
        if not e["stamp"].holds(*owners):
            if self.batched_epoch != _every and e["stamp"].intact(*owners):
                self.refresh_all(w.device, sync=True)
            if not e["stamp"].holds(*owners):     # written through ATen, replaced, or joined after this epoch's launch
                return self._single(e, w, scale, owners)
        # produced on ONE stream (the optimizer's for the batched refresh): a reader on another stream waits for it
        src = e["ev"] if e["ev"] is not None else self.ready
        if src is not None and w.is_cuda and torch.cuda.current_stream(w.device) != src[0]:
            torch.cuda.current_stream(w.device).wait_event(src[1])
        return e["wt"]

    def refresh_all(self, device, sync, trained_only=False):
        """every entry of this device by one launch, then (mode 4) every persistent operand's maximum by another.
        sync: from the middle of a step, where other streams may read the maxima; behind the optimizer none does"""
        from . import _C, amax
        # weights nobody asked for during the last two epochs belong to a model that is gone: dropped (with their buffers)
        for k in [k for k, e in self.entries.items() if e["used"] < _every - 2 or not e["stamp"].intact()]:
            del self.entries[k]
        live = [(k, e) for k, e in self.entries.items() if k[6] == device.index]
        self.batched_epoch = _every
        if live and (self.table is None or self.table[3] != [k for k, _ in live]):
            arr = (_lib.TransposeItem * len(live))()
            blocks = 0
            for i, (k, e) in enumerate(live):
                w_ptr, Cout, Cin, KH, KW, scale_ptr, _, cout_pad = k
                it = arr[i]
                it.w, it.scale, it.wt = w_ptr, scale_ptr or None, e["wt"].data_ptr()
                it.Cout, it.KH, it.KW, it.Cin = Cout, KH, KW, Cin
                it.cout_pad = cout_pad
                it.blocks_ci, it.blocks_co = (Cin + 31) // 32, (max(Cout, cout_pad) + 31) // 32
                it.first_block = blocks
                blocks += it.blocks_ci * it.blocks_co * KH * KW
            host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).clone()
            self.table = (host.to(device), len(live), blocks, [k for k, _ in live])
        if live:
            dev_t, n, blocks, _ = self.table
            _lib.call("dadet_conv_weight_transpose_batch", _p(dev_t), n, blocks, _stream())
        for _, e in live:
            e["stamp"].renew()
            e["ev"] = None
        if _C._mode4():
            amax.WEIGHTS.refresh(device, _every, sync=sync, trained_only=trained_only)
        if live and device.type == "cuda":
            st = torch.cuda.current_stream(device)
            self.ready = (st, st.record_event())


TRANSPOSES = _TransposeCache()


def bump(device=None, trained_only=False):
    """REQUIRED after any weight write that autograd's version counter does not see (the fused SGD kernel, `.data`: a
    broadcast, a checkpoint load, an EMA): the data-gradient GEMMs otherwise keep the transposed / padded copies of the
    old values and (contraction mode 4) the weight's old maximum — one that grew past twice of it overflows fp16 inside
    the GEMM and the step ends in inf / nan.  FusedSGD.step, BucketedGradReducer.broadcast_parameters and
    Checkpointer.load call it themselves.  With a device every transposed weight, then (mode 4) every maximum, is
    refreshed at once on the caller's stream (the optimizer's: behind the update and every reader of the old buffers);
    without one, at the first request.  trained_only=True (the optimizer): only tensors with requires_grad changed."""
    global _every, _full
    _every += 1
    if not trained_only:
        _full += 1
    if device is not None:
        TRANSPOSES.refresh_all(device, sync=False, trained_only=trained_only)
