"""The detection-loss kernels of csrc/losses.hip and fpn_merge_levels of csrc/sampling.hip called directly through their
`_C` wrappers, against float64 torch on the CPU (gradients from float64 autograd of the reference's own definition, at the
fp32 inputs the kernel saw) or, where the operation is a copy, against plain indexing.

Bars (tests/_bars.py, derived in tests/test_da_heads_gpu.py), u = 2^-24:
  a value that is one chain of operations:                16 u |ref| + one denormal step       (smooth-L1 gradients)
  a sum of n values of k leaves each:                     (n + k + 1 + 16) u S, S over the reference's leaves
    BCE term            max(x, 0) - x y + log1p(exp(-|x|))                3 leaves
    its gradient        (sigmoid(x) - y) / S                              2 leaves
    smooth-L1 term      0.5 d^2 / beta (one chain: x and t are exact fp32 values, so d = x - t carries one rounding of
                        its own value) or |d| - 0.5 beta                  2 leaves
    cross-entropy term  m + log(z) - x[label], z = sum_c exp(x_c - m)     3 leaves
    scatter-add         n = the number of rows meeting on the element     1 leaf
Cross entropy has one error source the two forms above do not describe: z is itself a sum of C positive terms, known to
(C + 1) u of its value whatever the order, and log turns that relative error into an ABSOLUTE (C + 2) u of every row's
term, however small the term is.  So the loss gets  + (C + 2) u  and a gradient element, (p_c - [c = label]) / n with
p_c = exp(x_c - lse), gets
      ((C + 20) u (p_c + [c = label]) + 2 u (|lse| + |x_c|) p_c) / n:
C + 2 from lse, 2 leaves + 16 as everywhere, and u (|lse| + |x_c|) twice because fp32 rounds lse = m + log z and the
difference x_c - lse to u of their magnitudes before exp turns that absolute error into a relative one (at a dominant
logit of 80 that term alone is 320 u: exp(x - 80) cannot be known better from fp32 operands).

BCE logits stay within +-3 for the bar cases, as tests/test_da_heads_gpu.py explains; one case goes to +-80 and is held to
the same leaf-sum bound.  Labels are exactly 0 / 1.  Smooth-L1 differences include exactly 0, exactly +-beta (x = beta as
fp32, t = 0), the fp32 neighbours of beta on both sides, and values well inside and outside.  No index, label or `keep`
value is out of range anywhere: defined behaviour only.

Every check prints its largest err / bound ratio."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _bars import FLOOR, U, check, elem_bound, f32, sum_bound

pytestmark = pytest.mark.gpu
CL = torch.channels_last


def _edges(beta32):
    """x - t of the first positives' values (t = 0): the first four are what a single positive gets"""
    b = np.float32(beta32)
    below, above = float(np.nextafter(b, np.float32(0))), float(np.nextafter(b, np.float32(2)))
    return torch.tensor([0.0, beta32, -beta32, below, above, -above, 0.5 * beta32, -0.25 * beta32, 1.5 * beta32,
                         -3.0 * beta32], dtype=torch.float32)


def _thrice(fn):
    first = fn()
    for _ in range(2):
        again = fn()
        for x, y in zip(first, again):
            assert torch.equal(x, y)
    return first


# ================================================================================================================ RPN
class _Rpn(object):
    """flat_o [T] logits and flat_r [T, 4] regression outputs in the order the losses are defined on; sampled int64 [S],
    the first Pn of them positive; labels [S]; tgt [Pn, 4]"""

    def __init__(self, seed, T, S, Pn, beta32, wide=False, pos_from=None, neg_from=None):
        g = torch.Generator().manual_seed(seed)
        self.T, self.S, self.Pn, self.beta = T, S, Pn, beta32
        self.flat_o = ((torch.rand(T, generator=g) * 2 - 1) * (80.0 if wide else 3.0)).float()
        self.flat_r = torch.randn(T, 4, generator=g)
        if pos_from is None:
            perm = torch.randperm(T, generator=g)[:S]
            pos, neg = perm[:Pn], perm[Pn:]
        else:
            pos = pos_from[torch.randperm(pos_from.numel(), generator=g)[:Pn]]
            rest = neg_from[~torch.isin(neg_from, pos)]
            neg = rest[torch.randperm(rest.numel(), generator=g)[:S - Pn]]
        assert pos.numel() == Pn and neg.numel() == S - Pn
        self.sampled = torch.cat([pos.sort().values, neg.sort().values])
        assert self.sampled.unique().numel() == S
        self.labels = torch.cat([torch.ones(Pn), torch.zeros(S - Pn)])
        self.tgt = torch.randn(Pn, 4, generator=g) * 0.3
        e = _edges(beta32)
        k = min(e.numel(), 4 * Pn)
        if k:
            at = torch.arange(k)
            self.tgt.view(-1)[:k] = 0.0
            self.flat_r[self.sampled[at // 4], at % 4] = e[:k]
        if wide and S >= 4:                       # both labels at both ends
            self.flat_o[self.sampled[0]], self.flat_o[self.sampled[1]] = 80.0, -80.0
            self.flat_o[self.sampled[-1]], self.flat_o[self.sampled[-2]] = 80.0, -80.0

    def reference(self):
        """binary_cross_entropy_with_logits over the sampled anchors, mean; smooth-L1 with beta over the positives, summed
        and divided by S; gradients by float64 autograd -> dict name -> (reference, bound)"""
        S, Pn, beta = self.S, self.Pn, self.beta
        o = self.flat_o.double().requires_grad_(True)
        r = self.flat_r.double().requires_grad_(True)
        y = self.labels.double()
        bce = F.binary_cross_entropy_with_logits(o[self.sampled], y)
        go, = torch.autograd.grad(bce, o)
        box, gr = torch.zeros((), dtype=torch.float64), torch.zeros_like(r)
        if Pn:
            box = F.smooth_l1_loss(r[self.sampled[:Pn]], self.tgt.double(), beta=beta, reduction="sum") / S
            gr, = torch.autograd.grad(box, r)
        with torch.no_grad():
            x = o[self.sampled]
            bce_leaves = (x.clamp(min=0) + (x * y).abs() + torch.log1p(torch.exp(-x.abs()))).sum() / S
            s = torch.sigmoid(x)
            b_go = torch.zeros(self.T, dtype=torch.float64)              # 0: an anchor not sampled gets exactly nothing
            b_go[self.sampled] = sum_bound(1, (s + y) / S, 2) + FLOOR
            d = (r[self.sampled[:Pn]] - self.tgt.double()).abs()
            box_leaves = torch.where(d < beta, 0.5 * d * d / beta, d + 0.5 * beta).sum() / S
            b_gr = torch.zeros_like(gr)
            b_gr[self.sampled[:Pn]] = elem_bound(gr[self.sampled[:Pn]])
        return {"bce": (bce.detach().reshape(1), sum_bound(S, bce_leaves, 3).reshape(1)),
                "box": (box.detach().reshape(1), sum_bound(max(4 * Pn, 1), box_leaves, 2).reshape(1)),
                "g_obj": (go, b_go), "g_reg": (gr, b_gr)}


def _maps(flat_o, flat_r, N, A, H, W, device):
    """[N, A, H, W] / [N, 4A, H, W] channels_last maps whose NHWC memory is the flat order (pixel, a) / (pixel, a, j)"""
    obj = flat_o.view(N, H, W, A).permute(0, 3, 1, 2).to(device).contiguous(memory_format=CL)
    reg = flat_r.reshape(N, H, W, 4 * A).permute(0, 3, 1, 2).to(device).contiguous(memory_format=CL)
    return obj, reg


def _check_rows(name, rows, pixels, a, pixel_want, go, gr, A):
    """rows [S, ldg] / pixels [S] against the reference gradient of every row's own anchor: go = (values [S], bounds [S]),
    gr = (values [S, 4], bounds [S, 4]).  Pad columns and the columns of the pixel's other anchors are exactly zero."""
    S, ldg = rows.shape
    assert ldg == (5 * A + 3) // 4 * 4
    rows, pixels = rows.cpu(), pixels.cpu()
    at = torch.arange(S)
    assert not bool(rows[:, 5 * A:].any()), name + ": a pad column was written"
    own = torch.zeros(S, ldg, dtype=torch.bool)
    want, bound = torch.zeros(S, ldg, dtype=torch.float64), torch.zeros(S, ldg, dtype=torch.float64)
    own[at, a], want[at, a], bound[at, a] = True, go[0], go[1]
    for j in range(4):
        own[at, A + 4 * a + j], want[at, A + 4 * a + j], bound[at, A + 4 * a + j] = True, gr[0][:, j], gr[1][:, j]
    assert not bool(rows[~own].any()), name + ": a row holds something outside its own anchor's 1 + 4 columns"
    assert torch.equal(pixels.long(), pixel_want), name + ": pixel index"
    check(name, rows, want, bound)


RPN_CASES = [
    # A, S, Pn, beta
    (15, 1, 0, 1.0), (15, 1, 1, 1.0 / 9), (15, 37, 0, 1.0 / 9), (15, 37, 1, 1.0), (15, 37, 37, 1.0 / 9),
    (15, 256, 70, 1.0 / 9), (15, 256, 256, 1.0), (15, 256, 1, 1.0 / 9),
    (15, 300, 70, 1.0), (15, 300, 300, 1.0 / 9), (15, 300, 0, 1.0),       # the second trip of both 256-lane loops
    (15, 512, 70, 1.0 / 9), (15, 512, 512, 1.0), (15, 512, 1, 1.0), (15, 512, 0, 1.0 / 9),
    (3, 1, 1, 1.0), (3, 37, 1, 1.0 / 9), (3, 37, 37, 1.0), (3, 200, 70, 1.0 / 9),     # ldg = 16: one pad column
    (1, 1, 0, 1.0 / 9), (1, 37, 1, 1.0), (1, 37, 37, 1.0 / 9), (1, 70, 70, 1.0),      # ldg = 8: three pad columns
]


def _rpn_dense_and_rows(device, p, N, A, H, W):
    from da_detect_amd import _C

    obj, reg = _maps(p.flat_o, p.flat_r, N, A, H, W, device)
    sd, ld, td = p.sampled.to(device), p.labels.to(device), p.tgt.to(device)
    losses, g_obj, g_reg = _thrice(lambda: _C.rpn_loss(obj, reg, sd, ld, sd[:p.Pn], td, p.beta))
    assert g_obj.shape == obj.shape and g_reg.shape == reg.shape
    r_losses, rows, pixels = _thrice(lambda: _C.rpn_loss_rows(obj, reg, sd, ld, p.Pn, td, p.beta))
    return (losses.cpu(), g_obj.permute(0, 2, 3, 1).reshape(-1).cpu(), g_reg.permute(0, 2, 3, 1).reshape(-1, 4).cpu(),
            r_losses.cpu(), rows.cpu(), pixels.cpu())


def _rpn_check_all(p, got, A):
    losses, g_obj, g_reg, r_losses, rows, pixels = got
    ref = p.reference()
    assert float(p.flat_o[p.sampled].abs().max()) <= 80.0
    check("loss_objectness", losses[:1], *ref["bce"])
    check("loss_rpn_box_reg", losses[1:], *ref["box"])
    if p.Pn == 0:
        assert float(losses[1]) == 0.0
    check("g_obj (zero bound off the sample)", g_obj, *ref["g_obj"])
    check("g_reg (zero bound off the positives)", g_reg, *ref["g_reg"])
    s = p.sampled
    _check_rows("rows", rows, pixels, s % A, s // A, (ref["g_obj"][0][s], ref["g_obj"][1][s]),
                (ref["g_reg"][0][s], ref["g_reg"][1][s]), A)
    # row form against dense form, bit for bit: the same arithmetic in the same order
    assert torch.equal(r_losses, losses)
    at, a = torch.arange(p.S), s % A
    so, sr = torch.zeros_like(g_obj), torch.zeros_like(g_reg)
    so[pixels.long() * A + a] = rows[at, a]
    for j in range(4):
        sr[pixels.long() * A + a, j] = rows[at, A + 4 * a + j]
    assert torch.equal(so, g_obj) and torch.equal(sr, g_reg)


@pytest.mark.parametrize("A,S,Pn,beta", RPN_CASES, ids=lambda v: "%.3g" % v)
def test_rpn_loss_dense_and_rows_against_float64(device, A, S, Pn, beta):
    """rpn_loss and rpn_loss_rows (plain form) on N = 2 maps of 5 x 7: losses and every gradient element within the bars,
    exact zeros everywhere else, rows == dense bit for bit, three calls bit-identical"""
    N, H, W = 2, 5, 7
    beta32 = f32(beta)
    p = _Rpn(1000 + 17 * A + S + Pn, N * H * W * A, S, Pn, beta32)
    assert float(p.flat_o.abs().max()) <= 3.0
    if Pn >= 3:
        d = (p.flat_r[p.sampled[:Pn]] - p.tgt).abs()
        assert bool((d == 0).any()) and bool((d == beta32).any()) and bool((d < beta32).any()) and bool((d > beta32).any())
    _rpn_check_all(p, _rpn_dense_and_rows(device, p, N, A, H, W), A)


def test_rpn_loss_logits_up_to_80_stay_finite_and_inside_the_leaf_bound(device):
    N, A, H, W, S, Pn = 2, 3, 5, 7, 37, 11
    p = _Rpn(77, N * H * W * A, S, Pn, f32(1.0 / 9), wide=True)
    x = p.flat_o[p.sampled]
    assert float(x.max()) == 80.0 and float(x.min()) == -80.0
    _rpn_check_all(p, _rpn_dense_and_rows(device, p, N, A, H, W), A)


LEVELS = [(5, 7), (3, 4), (2, 2)]
LEVEL_CASES = [
    # seed, S, Pn, levels of the positives, levels of all samples
    (1, 64, 20, (0, 1, 2), (0, 1, 2)),
    (2, 64, 10, (1,), (0, 1, 2)),              # every positive on one level
    (3, 40, 12, (0, 2), (0, 2)),               # level 1 receives no sample at all
    (4, 300, 70, (0, 1, 2), (0, 1, 2)),        # the second trip of both loops, 300 of the 306 anchors
    (5, 9, 0, (), (2,)),                       # no positive, everything on the coarsest level
]


@pytest.mark.parametrize("seed,S,Pn,pos_levels,all_levels", LEVEL_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_rpn_loss_rows_level_and_shared_forms(device, seed, S, Pn, pos_levels, all_levels):
    """three levels (5x7, 3x4, 2x2), N = 2, A = 3; sampled_inds index the image-major / level / (h, w, a) concatenation and
    the float64 reference is computed from the concatenated tensors"""
    from da_detect_amd import _C

    N, A = 2, 3
    cnt = [h * w * A for h, w in LEVELS]
    per_image = sum(cnt)
    off = [sum(cnt[:l]) for l in range(3)]
    level_of = torch.cat([torch.full((c,), l) for l, c in enumerate(cnt)]).repeat(N)          # [N * per_image]
    every = torch.arange(N * per_image)
    pos_from = every[torch.isin(level_of, torch.tensor(pos_levels, dtype=torch.long))]
    neg_from = every[torch.isin(level_of, torch.tensor(all_levels, dtype=torch.long))]
    beta32 = f32(1.0 / 9)
    p = _Rpn(4000 + seed, N * per_image, S, Pn, beta32, pos_from=pos_from, neg_from=neg_from)
    ref = p.reference()
    s = p.sampled
    lvl = level_of[s]
    rem = s % per_image - torch.tensor(off)[lvl]
    hw = torch.tensor([h * w for h, w in LEVELS])[lvl]
    a, pixel = rem % A, (s // per_image) * hw + rem // A
    if len(pos_levels) == 1:
        assert bool((lvl[:Pn] == pos_levels[0]).all())
    sd, ld, td = s.to(device), p.labels.to(device), p.tgt.to(device)
    maps = []
    for l, (h, w) in enumerate(LEVELS):
        fo = p.flat_o.view(N, per_image)[:, off[l]:off[l] + cnt[l]].reshape(-1)
        fr = p.flat_r.view(N, per_image, 4)[:, off[l]:off[l] + cnt[l]].reshape(-1, 4)
        maps.append(_maps(fo, fr, N, A, h, w, device))
    ldg = 16
    union = torch.zeros(S, ldg)
    union_pix = torch.full((S,), -9, dtype=torch.int32)
    total = torch.zeros(2, dtype=torch.float64)
    per_level = []
    for l in range(3):
        window = (per_image, off[l], cnt[l])
        losses, rows, pix = _thrice(lambda: _C.rpn_loss_rows(maps[l][0], maps[l][1], sd, ld, Pn, td, beta32, level=window))
        losses, rows, pix = losses.cpu(), rows.cpu(), pix.cpu()
        mine = lvl == l
        assert not bool(rows[~mine].any()) and bool((pix[~mine] == -1).all())      # other levels' rows: zero, pixel -1
        if not bool(mine.any()):
            assert float(losses[0]) == 0.0 and float(losses[1]) == 0.0
        if not bool(mine[:Pn].any()):
            assert float(losses[1]) == 0.0
        union[mine], union_pix[mine] = rows[mine], pix[mine]
        total += losses.double()
        per_level.append(losses)
    check("loss_objectness, levels added", total[:1], *ref["bce"])
    check("loss_rpn_box_reg, levels added", total[1:], *ref["box"])
    go, gr = (ref["g_obj"][0][s], ref["g_obj"][1][s]), (ref["g_reg"][0][s], ref["g_reg"][1][s])
    _check_rows("union of the levels' rows", union, union_pix, a, pixel, go, gr, A)
    # shared buffers: every launch writes and tags the rows of its own anchors only
    rows_s = torch.zeros(S, ldg, device=device)
    pix_s = torch.full((S,), -7, dtype=torch.int32, device=device)
    tag_s = torch.full((S,), -7, dtype=torch.int32, device=device)
    for l in range(3):
        before = (rows_s.clone(), pix_s.clone(), tag_s.clone())
        losses, r_out, p_out = _C.rpn_loss_rows(maps[l][0], maps[l][1], sd, ld, Pn, td, beta32,
                                                level=(per_image, off[l], cnt[l]), shared=(l, rows_s, pix_s, tag_s))
        assert r_out is rows_s and p_out is pix_s
        assert torch.equal(losses.cpu(), per_level[l])
        other = (lvl != l).to(device)
        for now, was in zip((rows_s, pix_s, tag_s), before):
            assert torch.equal(now[other], was[other])                            # untouched: another level's, or not yet
        mine = ~other
        assert bool((tag_s[mine] == l).all())
        assert bool((before[2][mine] == -7).all())                                 # written once: no earlier launch did
    assert torch.equal(tag_s.cpu().long(), lvl)
    assert torch.equal(rows_s.cpu(), union) and torch.equal(pix_s.cpu(), union_pix)


# ========================================================================================================= Fast R-CNN
class _Frcnn(object):
    def __init__(self, seed, R, C, agnostic, labels=None):
        g = torch.Generator().manual_seed(seed)
        self.R, self.C, self.agnostic = R, C, agnostic
        self.reg_cols = 8 if agnostic else 4 * C
        self.logits = torch.randn(R, C, generator=g) * 2
        self.reg = torch.randn(R, self.reg_cols, generator=g)
        self.tgt = torch.randn(R, 4, generator=g) * 0.5
        if labels is None:
            labels = torch.randint(1, C, (R,), generator=g)
            labels[torch.rand(R, generator=g) < 0.5] = 0                  # background
            labels[torch.rand(R, generator=g) < 0.4] = -1                 # rows outside the losses
            labels[-1] = C - 1                                            # the last row counts, with a box term
            if R >= 8:
                lab = C - 1
                labels[:6] = lab
                self.logits[0] = 0.0
                self.logits[0, lab] = 80.0                                # dominant logit on the label
                self.logits[1, 0] = 80.0                                  # dominant logit off the label
                self.logits[2, lab] = -80.0
                self.logits[3] = 1.25                                     # equal logits
                e = _edges(1.0)
                col0 = 4 if agnostic else 4 * lab
                self.tgt[4:6] = 0.0
                self.reg[4, col0:col0 + 4], self.reg[5, col0:col0 + 4] = e[:4], e[4:8]
        self.labels = labels

    def col0(self, lab):
        return torch.full_like(lab, 4) if self.agnostic else 4 * lab

    def reference(self):
        """cross_entropy over the rows that count, mean; smooth-L1 with beta 1 on the label's four columns, divided by the
        same count; float64 autograd -> dict name -> (reference, bound)"""
        R, C = self.R, self.C
        lg = self.logits.double().requires_grad_(True)
        rg = self.reg.double().requires_grad_(True)
        rows = torch.nonzero(self.labels >= 0).squeeze(1)
        n = rows.numel()
        lab = self.labels[rows]
        zero = torch.zeros((), dtype=torch.float64)
        ce, box = zero, zero
        g_cls, g_reg = torch.zeros_like(lg), torch.zeros_like(rg)
        b_cls, b_reg = torch.zeros_like(lg), torch.zeros_like(rg)
        b_ce, b_box = zero, zero
        pos = rows[lab > 0]
        cols = self.col0(self.labels[pos])[:, None] + torch.arange(4)
        if n:
            ce = F.cross_entropy(lg[rows], lab)
            g_cls, = torch.autograd.grad(ce, lg)
        if pos.numel():
            box = F.smooth_l1_loss(rg[pos[:, None], cols], self.tgt.double()[pos], beta=1.0, reduction="sum") / n
            g_reg, = torch.autograd.grad(box, rg)
        with torch.no_grad():
            if n:
                x = lg[rows]
                m = x.max(1).values
                lse = torch.logsumexp(x, 1)
                prob = torch.softmax(x, 1)
                hot = F.one_hot(lab, C).double()
                b_ce = sum_bound(n, (m.abs() + (lse - m).abs() + (x * hot).sum(1).abs()).sum() / n, 3) + (C + 2) * U
                b_cls[rows] = ((C + 20) * U * (prob + hot) + 2 * U * (lse.abs()[:, None] + x.abs()) * prob) / n + FLOOR
            if pos.numel():
                d = (rg[pos[:, None], cols] - self.tgt.double()[pos]).abs()
                b_box = sum_bound(4 * pos.numel(), torch.where(d < 1, 0.5 * d * d, d + 0.5).sum() / n, 2)
                b_reg[pos[:, None], cols] = elem_bound(g_reg[pos[:, None], cols])
        return {"ce": (ce.detach().reshape(1), torch.as_tensor(b_ce).reshape(1)),
                "box": (box.detach().reshape(1), torch.as_tensor(b_box).reshape(1)),
                "g_cls": (g_cls, b_cls), "g_reg": (g_reg, b_reg), "rows": rows, "pos": pos, "cols": cols}

    def run_rows(self, device):
        from da_detect_amd import _C

        args = (self.logits.to(device), self.reg.to(device), self.labels.to(device), self.tgt.to(device))
        return _thrice(lambda: _C.fast_rcnn_loss_rows(*args))

    def run_index(self, device, ref, seed):
        """the same problem through the index lists: src a permutation of the counted rows (in no order, with gaps)"""
        from da_detect_amd import _C

        g = torch.Generator().manual_seed(seed)
        src = ref["rows"][torch.randperm(ref["rows"].numel(), generator=g)]
        lab = self.labels[src]
        rows_pos = src[lab > 0]
        map_inds = (self.col0(self.labels[rows_pos])[:, None] + torch.arange(4)).contiguous()
        args = [v.to(device) for v in (self.logits, self.reg, src, lab, rows_pos, map_inds, self.tgt[rows_pos])]
        return _thrice(lambda: _C.fast_rcnn_loss(*args))


def _frcnn_check(tag, got, ref):
    losses, g_cls, g_reg = got
    check(tag + " loss_classifier", losses[:1], *ref["ce"])
    check(tag + " loss_box_reg", losses[1:], *ref["box"])
    check(tag + " g_cls (zero bound on ignored rows)", g_cls, *ref["g_cls"])
    check(tag + " g_reg (zero bound off the label's columns)", g_reg, *ref["g_reg"])


FRCNN_CASES = [
    # C, R, class-agnostic regression
    (2, 1, False), (9, 1, False), (81, 1, True),
    (2, 255, False), (2, 1000, True),              # C = 2: 8 columns are both 4 C and the class-agnostic 2 x 4
    (9, 255, True), (9, 256, False), (9, 257, True), (9, 512, False), (9, 1000, False),
    (81, 256, True), (81, 257, False), (81, 512, False), (81, 1000, True),
]


@pytest.mark.parametrize("C,R,agnostic", FRCNN_CASES, ids=lambda v: str(v))
def test_fast_rcnn_losses_against_float64(device, C, R, agnostic):
    """fast_rcnn_loss_rows and fast_rcnn_loss on the same problem: both within the bars of the float64 reference, and
    within one bar of each other; ignored rows and the regression columns of other classes exactly zero"""
    p = _Frcnn(2000 + C + R, R, C, agnostic)
    ref = p.reference()
    assert ref["rows"].numel() >= 1 and ref["pos"].numel() >= 1
    by_rows = p.run_rows(device)
    _frcnn_check("rows: ", by_rows, ref)
    by_index = p.run_index(device, ref, R)
    _frcnn_check("index:", by_index, ref)
    check("g_cls: rows against index", by_rows[1], by_index[1].double().cpu(), ref["g_cls"][1])
    check("g_reg: rows against index", by_rows[2], by_index[2].double().cpu(), ref["g_reg"][1])


@pytest.mark.parametrize("agnostic", [False, True], ids=["4C columns", "8 columns"])
def test_fast_rcnn_losses_count_edges(device, agnostic):
    """R = 257, C = 9.  All rows background: no box term, exactly.  All rows of a negative label: count 0, both losses and
    every gradient exactly 0, nothing non-finite.  Exactly one counted row, the last one (the second trip of the loop)."""
    R, C = 257, 9
    p = _Frcnn(31, R, C, agnostic, labels=torch.zeros(R, dtype=torch.int64))
    ref = p.reference()
    for got in (p.run_rows(device), p.run_index(device, ref, 1)):
        _frcnn_check("background:", got, ref)
        assert float(got[0][1]) == 0.0 and not bool(got[2].any())
    p = _Frcnn(32, R, C, agnostic, labels=torch.full((R,), -1, dtype=torch.int64))
    ref = p.reference()
    for got in (p.run_rows(device), p.run_index(device, ref, 2)):
        for v in got:
            assert bool(torch.isfinite(v).all()) and not bool(v.any())
    labels = torch.full((R,), -1, dtype=torch.int64)
    labels[R - 1] = 3
    p = _Frcnn(33, R, C, agnostic, labels=labels)
    ref = p.reference()
    assert ref["rows"].tolist() == [R - 1] and ref["pos"].tolist() == [R - 1]
    for got in (p.run_rows(device), p.run_index(device, ref, 3)):
        _frcnn_check("one row:", got, ref)


# ========================================================================================================= pixel taps
TAP_N, TAP_H, TAP_W = 2, 4, 5
#             four corners    edge interior image 2 (interior, corner) duplicate  neighbours  other level
TAP_PIXELS = [0, 4, 15, 19,   2,   7,       31, 39,                     7,         12, 13,     -1]


def _gather_ref(x, pixels, ksize, pad, rows=None):
    """x [N, C, H, W] -> [S, ksize^2, C] by plain indexing; rows: only these (the others stay NaN)"""
    N, C, H, W = x.shape
    out = torch.full((len(pixels), ksize * ksize, C), float("nan"), dtype=x.dtype)
    for r, p in enumerate(pixels):
        if rows is not None and r not in rows:
            continue
        out[r] = 0
        if p < 0:
            continue
        n, h0, w0 = p // (H * W), p % (H * W) // W, p % W
        for tap in range(ksize * ksize):
            h, w = h0 + tap // ksize - pad, w0 + tap % ksize - pad
            if 0 <= h < H and 0 <= w < W:
                out[r, tap] = x[n, :, h, w]
    return out


def _scatter_ref(y, pixels, shape, ksize, pad, rows=None):
    """-> (sum, sum of magnitudes, number of contributions) per element of the [N, C, H, W] map, float64"""
    N, C, H, W = shape
    dx, mag = torch.zeros(shape, dtype=torch.float64), torch.zeros(shape, dtype=torch.float64)
    cnt = torch.zeros(shape, dtype=torch.float64)
    for r, p in enumerate(pixels):
        if p < 0 or (rows is not None and r not in rows):
            continue
        n, h0, w0 = p // (H * W), p % (H * W) // W, p % W
        for tap in range(ksize * ksize):
            h, w = h0 + tap // ksize - pad, w0 + tap % ksize - pad
            if 0 <= h < H and 0 <= w < W:
                dx[n, :, h, w] += y[r, tap].double()
                mag[n, :, h, w] += y[r, tap].double().abs()
                cnt[n, :, h, w] += 1
    return dx, mag, cnt


@pytest.mark.parametrize("ksize,pad", [(1, 0), (3, 1)], ids=["1x1", "3x3"])
@pytest.mark.parametrize("C", [4, 5, 64, 1028], ids=lambda v: "C%d" % v)
def test_pixel_taps_gather_scatter_and_adjoint(device, C, ksize, pad):
    """gather is a copy: exact.  scatter adds with atomics: the sum bound with n = the contributions meeting on the element
    (0 of them: exactly zero).  <gather(x), y> == <x, scatter(y)> in float64 within the scatter's bound.  C = 1028: 257
    float4 for 256 lanes.  C = 5: scatter only (gather moves float4)."""
    from da_detect_amd import _C

    g = torch.Generator().manual_seed(C * 10 + ksize)
    N, H, W = TAP_N, TAP_H, TAP_W
    S, T = len(TAP_PIXELS), ksize * ksize
    x = torch.randn(N, C, H, W, generator=g)
    y = torch.randn(S, T, C, generator=g)
    pix = torch.tensor(TAP_PIXELS, dtype=torch.int32, device=device)
    dx = _C.scatter_pixel_taps_add(y.to(device), pix, (N, C, H, W), ksize, pad)
    assert tuple(dx.shape) == (N, C, H, W)
    want, mag, cnt = _scatter_ref(y, TAP_PIXELS, (N, C, H, W), ksize, pad)
    assert float(cnt.max()) >= (2 if ksize == 1 else 4) and float(cnt.min()) == 0
    check("scatter", dx, want, sum_bound(cnt, mag))
    if C % 4:
        return
    got = _C.gather_pixel_taps(x.to(device).contiguous(memory_format=CL), pix, ksize, pad)
    assert tuple(got.shape) == (S, T, C)
    assert torch.equal(got.cpu(), _gather_ref(x, TAP_PIXELS, ksize, pad))
    lhs = (got.double().cpu() * y.double()).sum()
    rhs = (x.double() * dx.double().cpu()).sum()
    check("adjoint identity", rhs.reshape(1), lhs.reshape(1), (x.double().abs() * sum_bound(cnt, mag)).sum().reshape(1))


@pytest.mark.parametrize("ksize,pad", [(1, 0), (3, 1)], ids=["1x1", "3x3"])
def test_pixel_taps_level_forms_touch_only_their_rows(device, ksize, pad):
    from da_detect_amd import _C

    g = torch.Generator().manual_seed(5 + ksize)
    N, C, H, W = TAP_N, 8, TAP_H, TAP_W
    S, T = len(TAP_PIXELS), ksize * ksize
    x = torch.randn(N, C, H, W, generator=g)
    y = torch.randn(S, T, C, generator=g)
    tags = [r % 3 for r in range(S)]
    tags[-1] = 1                                   # the -1 row is tagged with the level under test: written, as zeros
    pix = torch.tensor(TAP_PIXELS, dtype=torch.int32, device=device)
    row_level = torch.tensor(tags, dtype=torch.int32, device=device)
    mine = [r for r in range(S) if tags[r] == 1]
    out = torch.full((S, T, C), 7.0, device=device)
    back = _C.gather_pixel_taps(x.to(device).contiguous(memory_format=CL), pix, ksize, pad, row_level=row_level, level=1,
                                out=out)
    assert back is out
    want = _gather_ref(x, TAP_PIXELS, ksize, pad, rows=mine)
    want[want.isnan()] = 7.0                      # rows tagged with another level keep their fill
    assert torch.equal(out.cpu(), want)
    dx = _C.scatter_pixel_taps_add(y.to(device), pix, (N, C, H, W), ksize, pad, row_level=row_level, level=1)
    ref, mag, cnt = _scatter_ref(y, TAP_PIXELS, (N, C, H, W), ksize, pad, rows=mine)
    check("scatter, level 1 only", dx, ref, sum_bound(cnt, mag))


def test_pixel_taps_empty_and_refusal(device):
    from da_detect_amd import _C, _lib

    x = torch.randn(2, 8, 4, 5).to(device).contiguous(memory_format=CL)
    none = torch.empty(0, dtype=torch.int32, device=device)
    assert tuple(_C.gather_pixel_taps(x, none, 3, 1).shape) == (0, 9, 8)
    dx = _C.scatter_pixel_taps_add(torch.empty((0, 9, 8), device=device), none, (2, 8, 4, 5), 3, 1)
    assert tuple(dx.shape) == (2, 8, 4, 5) and not bool(dx.any())
    x6 = torch.randn(2, 6, 4, 5).to(device).contiguous(memory_format=CL)
    with pytest.raises(_lib.DadetError):
        _C.gather_pixel_taps(x6, torch.zeros(3, dtype=torch.int32, device=device), 1, 0)


# =================================================================================================== fpn_merge_levels
def _merge_level(g, n, count, device):
    xy = torch.rand(n, 2, generator=g) * 100
    boxes = torch.cat([xy, xy + 1 + torch.rand(n, 2, generator=g) * 50], 1)
    scores = torch.rand(n, generator=g).sort(descending=True).values
    keep = torch.randperm(n, generator=g).sort().values if n else torch.empty(0, dtype=torch.int64)
    if n > 3:
        keep = torch.randperm(n, generator=g)                       # any in-range positions, not only ascending ones
    cnt = torch.tensor([count], dtype=torch.int32)
    return (boxes, scores, keep, cnt), tuple(v.to(device) for v in (boxes, scores, keep, cnt))


def _merge_check(levels_cpu, post_n, boxes_out, scores_out):
    off = 0
    boxes_out, scores_out = boxes_out.cpu(), scores_out.cpu()
    for boxes, scores, keep, cnt in levels_cpu:
        cap = min(boxes.shape[0], post_n)
        kept = min(int(cnt), cap)
        idx = keep[:kept]
        assert torch.equal(boxes_out[off:off + kept], boxes[idx]) and torch.equal(scores_out[off:off + kept], scores[idx])
        assert bool((scores_out[off + kept:off + cap] == -1.0).all())                 # behind the kept count
        if cap > kept:
            assert torch.equal(boxes_out[off + kept:off + cap], boxes[:1].expand(cap - kept, 4))
        off += cap                                                                     # the next level's running offset
    assert boxes_out.shape[0] == off and scores_out.shape[0] == off


@pytest.mark.parametrize("post_n", [1, 256, 257, 1000], ids=lambda v: "post_n%d" % v)
@pytest.mark.parametrize("rot", [0, 1, 2, 3], ids=lambda v: "counts%d" % v)
def test_fpn_merge_levels_equals_indexing(device, post_n, rot):
    """two images x three levels with n in {0, 1, 300, 1000} candidates; every level's count is one of 0, 1, cap, above
    cap (the parameter `rot` moves the four through the levels)"""
    from da_detect_amd import _C

    g = torch.Generator().manual_seed(post_n + rot)
    sizes = [[300, 0, 1000], [1, 1000, 300]]
    cpu, dev, k = [], [], rot
    for ns in sizes:
        lc, ld = [], []
        for n in ns:
            cap = min(n, post_n)
            count = [0, 1, cap, cap + 5][k % 4] if n else 0
            k += 1
            c, d = _merge_level(g, n, min(count, n), device)
            lc.append(c)
            ld.append(d)
        cpu.append(lc)
        dev.append(ld)
    outs = _C.fpn_merge_levels(dev, post_n)
    assert len(outs) == 2
    for lc, (b, s) in zip(cpu, outs):
        _merge_check(lc, post_n, b, s)


def test_fpn_merge_levels_crosses_the_wrapper_chunk(device):
    """9 images x 3 levels = 27 (level, image) pairs: two launches of at most 24"""
    from da_detect_amd import _C

    g = torch.Generator().manual_seed(9)
    cpu, dev = [], []
    for i in range(9):
        pairs = [_merge_level(g, n, (i + n) % (n + 1), device) for n in (5, 2, 7)]
        cpu.append([c for c, _ in pairs])
        dev.append([d for _, d in pairs])
    outs = _C.fpn_merge_levels(dev, 3)
    for lc, (b, s) in zip(cpu, outs):
        _merge_check(lc, 3, b, s)
