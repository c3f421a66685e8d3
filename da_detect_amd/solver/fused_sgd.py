"""SGD with momentum as ONE multi-tensor HIP launch per step.

Numerically torch.optim.SGD (dampening 0, no nesterov): d = g + wd * p; buf = d (first step) or
momentum * buf + d; p -= lr * buf — applied to the reference's one-param-group-per-tensor layout
(reference: maskrcnn_benchmark/solver/build.py:7-20, engine/trainer.py:237-239) by dadet_sgd_step, which reads a
device-resident table of (p, g, buf, numel, lr, weight_decay) entries.  It subclasses torch.optim.Optimizer so
LR schedulers and checkpoint code that walk `param_groups` / `state_dict()` keep working.
"""
import collections
import ctypes
import os

import torch

from .. import _lib
from .._lib import SgdEntry

# what one step launches from: `rows` of (p, g, buf, numel, lr, weight decay) as uploaded to `table`, and one
# (first row, rows, largest numel) range per gradient bucket (by_bucket) or one over everything
_Plan = collections.namedtuple("_Plan", "by_bucket rows table ranges device momentum")


class FusedSGD(torch.optim.Optimizer):
    def __init__(self, params, lr, momentum=0.0, weight_decay=0.0):
        defaults = dict(lr=lr, momentum=momentum, weight_decay=weight_decay)
        super(FusedSGD, self).__init__(params, defaults)
        self._plan = self._bucket_plan = None     # the last step's _Plan: kept while the rows stay what they are
        self._stage = None       # two (pinned host buffer, device buffer, event): the table of step t lives in t % 2
        self._steps = 0
        self.reducer = None      # optional parallel.reducer.BucketedGradReducer owning the .grad storage
        # one update launch per gradient bucket as its collective completes (several ranks); DADET_SGD_PER_BUCKET=0: one
        # launch behind all collectives
        self.per_bucket = os.environ.get("DADET_SGD_PER_BUCKET", "1") == "1"

    def attach_reducer(self, reducer):
        """gradients live in the reducer's flat buckets: zero_grad() clears them in place (stable pointers)
        and step() first completes the outstanding all-reduces"""
        self.reducer = reducer
        # with persistent zeroed .grad buffers the weight-gradient kernels may accumulate into them directly
        from ..utils import streams
        streams.enable_direct_wgrad(True)

    def zero_grad(self, set_to_none=True):
        if self.reducer is not None:
            self.reducer.zero_grad()
        else:
            super(FusedSGD, self).zero_grad(set_to_none=set_to_none)

    def _entries(self):
        out = []
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                # with the reducer every .grad is a persistent (zeroed) bucket view: a parameter that received no
                # gradient this step must still be SKIPPED, as torch.optim.SGD skips `grad is None` (no weight decay,
                # no momentum update) — e.g. the instance head when its loss weight is 0
                # (with several ranks: no gradient on ANY rank — reducer.update_ids)
                if self.reducer is not None and id(p) not in self._update_ids:
                    continue
                out.append((p, group["lr"], group["weight_decay"], group["momentum"]))
        return out

    def _make_plan(self, by_bucket):
        """this step's _Plan (None: nothing to update).  by_bucket: rows ordered by the reducer's buckets, one range each"""
        entries = self._entries()
        if not entries:
            return None
        momentum = entries[0][3]
        assert all(e[3] == momentum for e in entries), "FusedSGD: one momentum for all groups"
        if by_bucket:
            buckets = self.reducer.buckets
            order = {id(p): i for i, b in enumerate(buckets) for p in b["params"]}
            entries.sort(key=lambda e: order.get(id(e[0]), len(buckets)))
            if id(entries[-1][0]) not in order:
                raise _lib.DadetError("FusedSGD: a parameter outside the reducer's buckets cannot be updated bucket by bucket")
            owner = [order[id(e[0])] for e in entries]
        rows = []
        for p, lr, wd, _ in entries:
            if not p.is_cuda:
                raise _lib.DadetError("FusedSGD runs on the HIP device only")
            g = p.grad
            if g.stride() != p.stride() or not _dense(p):
                # the kernel walks raw storage: gradient must share the parameter's physical layout
                if self.reducer is not None:      # a view of a bucket: replacing it would take it out of the collectives
                    index = [id(q) for group in self.param_groups for q in group["params"]].index(id(p))
                    raise _lib.DadetError("FusedSGD: parameter %d, shape %s strides %s, has a gradient of strides %s in the "
                                          "reducer's bucket: the update needs both dense and in one layout"
                                          % (index, tuple(p.shape), p.stride(), g.stride()))
                g = p.grad = torch.empty_strided(p.size(), p.stride(), dtype=g.dtype, device=g.device).copy_(g)
            st = self.state[p]
            if "momentum_buffer" not in st:
                # a zero buffer makes the general update `buf = momentum * buf + d` equal torch's first-step rule
                # `buf = d` exactly, also for a parameter that joins later (first gradient after some steps)
                st["momentum_buffer"] = torch.empty_strided(p.size(), p.stride(), dtype=p.dtype,
                                                            device=p.device).zero_()
            rows.append((p.data_ptr(), g.data_ptr(), st["momentum_buffer"].data_ptr(), p.numel(), lr, wd))
        rows = tuple(rows)
        plan = self._plan
        if plan is None or plan.by_bucket != by_bucket or plan.rows != rows:
            if by_bucket:
                ranges = [(0, 0, 0)] * len(buckets)
                for i, o in enumerate(owner):
                    first, n, largest = ranges[o]
                    ranges[o] = (first if n else i, n + 1, max(largest, rows[i][3]))
            else:
                ranges = [(0, len(rows), max(r[3] for r in rows))]
            device = entries[0][0].device
            plan = self._plan = _Plan(by_bucket, rows, self._upload(rows, device), ranges, device, momentum)
            self._bucket_plan = plan if by_bucket else None      # (the name the per-bucket plan had: [3] are the ranges)
        return plan

    def _upload(self, rows, device):
        """The table changes every step under a per-iteration schedule (the cosine schedule of the reference's trainer
        rewrites every group's lr): it is staged in one of two pinned host buffers and uploaded on the compute stream
        without blocking the host (a pageable `.to(device)` here stalled the host once per step until the stream had
        drained); the kernel of step t reads device copy t % 2."""
        arr = (SgdEntry * len(rows))()
        for i, r in enumerate(rows):
            arr[i].p, arr[i].g, arr[i].buf, arr[i].numel, arr[i].lr, arr[i].weight_decay = r
        nbytes = ctypes.sizeof(arr)
        if self._stage is None or self._stage[0][0].numel() != nbytes:
            self._stage = [(torch.empty(nbytes, dtype=torch.uint8).pin_memory(),
                            torch.empty(nbytes, dtype=torch.uint8, device=device),
                            torch.cuda.Event()) for _ in range(2)]
        host, dev, done = self._stage[self._steps % 2]
        done.synchronize()            # the upload issued two steps ago from this buffer (long finished)
        ctypes.memmove(host.data_ptr(), ctypes.addressof(arr), nbytes)
        dev.copy_(host, non_blocking=True)
        done.record()
        return dev

    def _step_bucket(self, plan, index, grad_scale):
        """the update of the tensors in range `index` of the plan: one gradient bucket's, or everything"""
        first, n, max_numel = plan.ranges[index]
        if n:
            _lib.call("dadet_sgd_step", ctypes.c_void_p(plan.table.data_ptr() + first * ctypes.sizeof(SgdEntry)), n,
                      ctypes.c_int64(max_numel), float(plan.momentum), 0, float(grad_scale),
                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        red = self.reducer
        # the 1 / world of the gradient mean rides in the kernel's gradient read (g * grad_scale: exact for the
        # power-of-two worlds of one node) instead of one multiply launch per bucket
        if red is not None and self.per_bucket and red.can_hand_over_buckets():
            # (round 6) one SGD launch per gradient bucket, issued as that bucket's all-reduce completes: the last
            # bucket's collective — the exposed tail of a ~6 ms backward — runs beside the earlier buckets' updates.
            # The plan is made before the waits: between them the callback only indexes it
            self._update_ids = red.update_ids()
            plan = self._make_plan(by_bucket=True)
            scale = grad_scale / red.world_size
            red.finalize(mean=False, per_bucket=lambda i, b: plan is not None and self._step_bucket(plan, i, scale))
            self._steps += 1
        else:
            if red is not None:
                red.finalize(mean=False)
                grad_scale = grad_scale * red.mean_scale
                self._update_ids = red.update_ids()
            plan = self._make_plan(by_bucket=False)
            if plan is not None:
                self._step_bucket(plan, 0, grad_scale)
                self._steps += 1
        if plan is not None:
            from .. import _C
            # parameters changed through raw pointers: the cached transposed weights are refreshed here, in one launch
            # (trained_only: frozen weights did not change — their maxima are not re-measured)
            _C.bump_weight_epoch(plan.device, trained_only=True)
        return loss


def _dense(t):
    return t.is_contiguous() or t.is_contiguous(memory_format=torch.channels_last)
