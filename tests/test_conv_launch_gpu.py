"""Every kernel family of the convolution plans (csrc/conv_plan.h) launches what it launched before the plan layer existed.

One case per forward / weight-gradient family — the smallest descriptor of tests/golden/conv_plans.npz that the recorded
plan assigns to it (at most 80 000 GEMM rows; dense gy rows and Cout % 4 == 0 for the weight gradient), under the setting
the fixture recorded it with — plus the paths inside the families: the symmetric two-part meeting of the large tile, three
parts, the tail cut, split-K under a full epilogue (scale, bias, addend, gate), a grouped weight gradient on 256 x 256 and
one on 128 x 128 tiles.  Each case runs once on inputs from a seeded CPU generator; the SHA-256 of the output bytes (and of
the published output maximum in contraction mode 4) must equal what this same code gave with the library of the commit
before the plan layer, on an MI355X, twice (tests/golden/conv_launch_hashes.json).  Accuracy is the business of the float64
tests in test_conv_big_gpu.py / test_ops_gpu.py; this one says that kernel, grid, arguments and scratch layout did not move."""
import hashlib
import json
import os
import struct

import numpy as np
import pytest
import torch

from tests.golden import make_conv_plans as G

pytestmark = pytest.mark.gpu
CL = torch.channels_last
HERE = os.path.dirname(os.path.abspath(__file__))
MAX_ROWS = 80000


def _cases():
    z = np.load(os.path.join(HERE, "golden", "conv_plans.npz"))
    desc, setting = z["desc"].astype(np.int64), z["setting"]
    nd = len(desc)
    didx = np.arange(len(setting)) % nd
    M = (desc[:, 0] * desc[:, 9] * desc[:, 10])[didx]
    work = M * (desc[:, 3] * desc[:, 4] * desc[:, 5] * desc[:, 6])[didx]
    settings = json.loads(str(z["settings"]))
    mode = np.asarray([s[0] for s in settings])[setting]

    def smallest(mask, what):
        i = np.nonzero(mask & (M > 0) & (M <= MAX_ROWS))[0]       # (an empty batch launches nothing)
        assert len(i), what
        i = i[np.lexsort((i, mode[i] != 4, work[i]))[0]]    # least work; ties: the default contraction, then fixture order
        return tuple(int(v) for v in desc[didx[i]]), settings[setting[i]]

    fwd_ok = z["fwd_rc"] == 0
    cases = []
    for f, name in enumerate(G.FWD_FAMILIES):
        cases.append(("fwd_" + name, "fwd") + smallest(fwd_ok & (z["fwd_family"] == f), name))
    big = fwd_ok & (z["fwd_family"] == G.FWD_FAMILIES.index("big256"))
    cases.append(("fwd_big256_two_part_meeting", "fwd") + smallest(big & (z["fwd_big_splits"] == 2) & (z["fwd_big_body"] == 0), "2"))
    cases.append(("fwd_big256_three_parts", "fwd") + smallest(big & (z["fwd_big_splits"] == 3), "3"))
    cases.append(("fwd_big256_tail_cut", "fwd") + smallest(big & (z["fwd_big_body"] > 0), "tail"))
    cases.append(("fwd_split_k_full_epilogue", "fwd_full")
                 + smallest(fwd_ok & (z["fwd_family"] == G.FWD_FAMILIES.index("split_k")), "split-K"))
    dense4 = (desc[:, 4] % 4 == 0)[didx]
    for f, name in enumerate(G.WGRAD_FAMILIES):
        cases.append(("wgrad_" + name, "wgrad") + smallest(dense4 & (z["wgrad_family"] == f), name))
    default = [4, 1, {}]
    for gi, kind in ((0, 256), (1, 128)):
        assert int(z["group_kind"][settings.index(default) * len(G.GROUPS) + gi]) == kind
        cases.append(("wgrad_group_%d" % kind, "group", G.GROUPS[gi], default))
    return cases


CASES = _cases()


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _randn(g, shape, device, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(device).contiguous(memory_format=CL)


def run_case(case, device):
    """-> {name: sha256} of everything the case's launches wrote"""
    from da_detect_amd import _C, _lib, amax

    cid, kind, what, (mode, big, env) = case
    lib = _lib.load()
    prev_mode, prev_big = _C.get_gemm_mode(), lib.dadet_get_big_gemm()
    saved = {k: os.environ.get(k) for k in env}
    g = torch.Generator().manual_seed(int(hashlib.sha256(cid.encode()).hexdigest()[:8], 16))
    out = {}
    try:
        _C.set_gemm_mode(mode)
        lib.dadet_set_big_gemm(big)
        os.environ.update(env)
        if kind == "group":
            reqs = []
            for N, H, W, Cin, Cout, k, stride in what:
                reqs.append(dict(x=_randn(g, (N, Cin, H, W), device), gy=_randn(g, (N, Cout, H, W), device),
                                 weight_shape=(Cout, Cin, k, k), stride=stride, pad=k // 2,
                                 dw=torch.empty((Cout, Cin, k, k), device=device).contiguous(memory_format=CL)))
            pending = _C.WgradBatch()
            assert _C.conv_wgrad_group(reqs, pending)
            _C.conv_wgrad_reduce_batch(pending)
            for i, r in enumerate(reqs):
                out["dw%d" % i] = _sha(r["dw"])
            return out
        N, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo = what
        x = _randn(g, (N, Cin, H, W), device)
        if kind == "wgrad":
            gy = _randn(g, (N, Cout, Ho, Wo), device)
            out["dw"] = _sha(_C.conv_wgrad(x, gy, (Cout, Cin, KH, KW), stride=stride, pad=pad))
            return out
        w = _randn(g, (Cout, Cin, KH, KW), device, (2.0 / (Cin * KH * KW)) ** 0.5)
        kw = {}
        if kind == "fwd_full":
            kw = dict(scale=(torch.rand(Cout, generator=g) + 0.5).to(device), bias=torch.randn(Cout, generator=g).to(device),
                      addend=_randn(g, (N, Cout, Ho, Wo), device), relu_mode=2,
                      mask_ref=_randn(g, (N, Cout, Ho, Wo), device).clamp_min(0))
        y = _C.conv_forward(x, w, stride=stride, pad=pad, out_size=(Ho, Wo), **kw)
        out["y"] = _sha(y)
        if mode == 4:
            out["amax_y"] = hashlib.sha256(struct.pack("<f", amax.value(y))).hexdigest()
        return out
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        lib.dadet_set_big_gemm(prev_big)
        _C.set_gemm_mode(prev_mode)


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(HERE, "golden", "conv_launch_hashes.json")) as f:
        return json.load(f)


def test_every_family_and_path_has_a_recorded_case(recorded):
    # at most two cases may be missing from the hashed set (not reproducible before the plan layer either)
    missing = [c[0] for c in CASES if c[0] not in recorded["hashes"]]
    assert sorted(missing) == sorted(recorded["not_reproducible"]) and len(missing) <= 2, missing


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_launch_writes_the_recorded_bits(device, recorded, case):
    got = run_case(case, device)
    from da_detect_amd import _C

    _C.check_nonfinite()
    if case[0] in recorded["not_reproducible"]:
        return          # ran (no fault, finite); its bits differ from run to run at the recorded commit too
    assert got == recorded["hashes"][case[0]], (case, got)
