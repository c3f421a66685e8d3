"""Records what the convolution plan queries of libdadet_hip.so answer over a grid of descriptors and settings:
tests/golden/conv_plans.npz (integer columns and names only).  Pure host code: needs the built library, no GPU.

    python tests/golden/make_conv_plans.py [--lib path/to/libdadet_hip.so] [--out tests/golden/conv_plans.npz]

The committed fixture was recorded from the commit BEFORE the plan layer (csrc/conv_plan.h) existed, through two throw-away
entry points with the signatures of dadet_conv_forward_plan / dadet_conv_wgrad_plan that called that commit's own planning
functions in the order its launch code did.  tests/test_conv_plan.py runs record() against the current library and compares
row by row.  `fwd_name` / `wgrad_name` in the fixture are the labels the Python binding of that commit derived from the
legacy variant queries (parent_fwd_name / parent_wgrad_name below, kept here as the reference).
"""
import argparse
import ctypes
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FWD_FAMILIES = ("exact", "split", "split_streamk", "split_k", "weight_stationary", "big256", "big128")
WGRAD_FAMILIES = ("exact", "split", "split_small_map", "big256")

DESC_FIELDS = ("N", "H", "W", "Cin", "Cout", "KH", "KW", "stride", "pad", "Ho", "Wo")
from da_detect_amd._lib import ConvDesc, ConvPlanInfo  # noqa: E402

INFO_FIELDS = tuple(n for n, _ in ConvPlanInfo._fields_ if n != "name")       # every integer field of the plan


# (gemm mode, big_gemm, {per-call switch: value})
SETTINGS = [(m, b, {}) for m in (0, 3, 4) for b in (0, 1, 2)] + [
    (4, 1, {"DADET_STREAMK": "0"}), (4, 1, {"DADET_STREAMK_SMALL": "1"}), (4, 1, {"DADET_WS_1X1": "0"}),
    (4, 1, {"DADET_WS_K256_BN": "64"}), (4, 1, {"DADET_BIG_SPLITS": "3"}), (4, 1, {"DADET_BIG_TAIL": "0"}),
    (4, 2, {"DADET_BIG_TILE_N": "128"}), (4, 1, {"DADET_WGRAD_SPLITS": "5"}), (4, 1, {"DADET_WGRAD_BIG_SPLITS": "4"}),
    (4, 1, {"DADET_WGRAD_GROUP_ROWS": "128"}), (4, 1, {"DADET_WGRAD_MIN_ROWS": "64"}), (4, 1, {"DADET_EPILOGUE_V4": "0"})]
SWITCHES = sorted({k for _, _, env in SETTINGS for k in env})

MAPS = ((2, 256, 512), (2, 128, 256), (2, 64, 128), (2, 32, 64), (3, 64, 128), (256, 7, 7), (512, 7, 7), (256, 14, 14),
        (512, 14, 14), (1, 8, 8), (1, 128, 257), (2, 200, 330))
CINS = (64, 128, 256, 512, 1024, 2048)
COUTS = (18, 32, 64, 128, 132, 256, 260, 512, 1024, 2048)
# three groups of tests/test_host_logic.py: (N, H, W, Cin, Cout, k, stride), pad = k // 2, output = input size
GROUPS = (((2, 64, 128, 256, 1024, 1, 1), (2, 64, 128, 256, 256, 3, 1), (2, 64, 128, 1024, 256, 1, 1)),
          ((2, 128, 256, 128, 512, 1, 1), (2, 128, 256, 128, 128, 3, 1), (2, 128, 256, 512, 128, 1, 1)),
          ((512, 7, 7, 2048, 512, 1, 1), (512, 7, 7, 512, 512, 3, 1), (512, 7, 7, 512, 2048, 1, 1)))


def descriptors():
    """the grid as rows of DESC_FIELDS (the whole cross product fits the fixture's size bound of 256 KB and reaches every
    kernel family)"""
    rows = []
    for (N, H, W), Cin, Cout, k, stride in itertools.product(MAPS, CINS, COUTS, (1, 3), (1, 2)):
        pad = k // 2
        rows.append((N, H, W, Cin, Cout, k, k, stride, pad, (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1))
    rows.append((2, 256, 512, 4, 64, 7, 8, 2, 3, 128, 256))        # the stem: a 7 x 7 kernel zero-padded to 7 x 8
    rows.append((0, 7, 7, 512, 512, 3, 3, 1, 1, 7, 7))             # an empty batch (no ROIs): nothing launches, the queries answer
    return rows


def parent_fwd_name(variant, mode, Cin, Cout, env):
    """the forward label as the Python binding derived it from dadet_conv_forward_variant before the plan layer"""
    if variant == 4:
        return "conv_big_kernel<256>"
    if variant == 5:
        return "conv_big128_kernel"
    if variant == 3:
        bn = 128
        if Cin == 256:
            wide = mode == 4 and Cout >= 256 and env.get("DADET_WS_K256_BN", "") != "64"
            bn = 128 if wide else 64
        return "conv1x1_ws_kernel<%d,%d,%d>" % (Cin, bn, mode)
    return ("conv_fwd_kernel<%s>" if mode == 0 else ("conv_fwd_split_kernel<%%s,%d>" % mode)) % ("2,2", "2,1", "1,1")[variant]


def parent_wgrad_name(variant, mode, dense_rows):
    if mode == 0:
        return "conv_wgrad_kernel"
    if dense_rows and variant == 1:
        return "conv_wgrad_big_kernel"
    return "conv_wgrad_split_kernel<%d>" % mode


def record(lib, rows, names_from_plan):
    """-> dict of arrays: one row per (setting, descriptor).  names_from_plan: take the labels from the plan entry points
    (the current library); otherwise derive them the parent's way from the legacy queries."""
    mode0, big0 = lib.dadet_get_gemm_mode(), lib.dadet_get_big_gemm()
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    cols = {k: [] for k in ("setting", "fwd_rc", "legacy_fwd_variant", "legacy_wgrad_variant", "legacy_wgrad_bytes")}
    for pre in ("fwd_", "wgrad_", "wgradld_"):
        for f in INFO_FIELDS:
            cols[pre + f] = []
    names = {"fwd_name": [], "wgrad_name": [], "wgradld_name": []}
    group_cols = {k: [] for k in ("setting", "group", "kind", "splits", "bytes")}
    info = ConvPlanInfo()
    try:
        for si, (mode, big, env) in enumerate(SETTINGS):
            assert lib.dadet_set_gemm_mode(mode) == 0 and lib.dadet_set_big_gemm(big) == 0
            os.environ.update(env)
            for row in rows:
                N, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo = row
                d = ConvDesc(N, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo, Ho, Wo, 1, 0)
                cols["setting"].append(si)
                lfv = lib.dadet_conv_forward_variant(ctypes.byref(d))
                # (an empty batch under big_gemm 2: the commit the fixture was recorded from divided by zero in this query)
                lwv = -2 if (N == 0 and mode == 4 and big == 2) else lib.dadet_conv_wgrad_variant(ctypes.byref(d))
                nbytes = ctypes.c_size_t(0)
                assert lib.dadet_conv_wgrad_workspace_bytes(ctypes.byref(d), ctypes.byref(nbytes)) == 0, row
                cols["legacy_fwd_variant"].append(lfv)
                cols["legacy_wgrad_variant"].append(lwv)
                cols["legacy_wgrad_bytes"].append(nbytes.value)
                rc = lib.dadet_conv_forward_plan(ctypes.byref(d), ctypes.byref(info))
                cols["fwd_rc"].append(rc)
                for f in INFO_FIELDS:
                    cols["fwd_" + f].append(getattr(info, f) if rc == 0 else -1)
                if rc != 0:
                    names["fwd_name"].append("")
                else:
                    names["fwd_name"].append(info.name.decode() if names_from_plan
                                             else parent_fwd_name(lfv, mode, Cin, Cout, env))
                # gy_ld: Cout, and Cout rounded up to a multiple of four where that is another value (wgradld_*; those rows only)
                for pre, gy_ld in (("wgrad_", Cout), ("wgradld_", (Cout + 3) // 4 * 4)):
                    if pre == "wgradld_" and gy_ld == Cout:
                        continue
                    assert lib.dadet_conv_wgrad_plan(ctypes.byref(d), gy_ld, ctypes.byref(info)) == 0, row
                    for f in INFO_FIELDS:
                        cols[pre + f].append(getattr(info, f))
                    names[pre + "name"].append(info.name.decode() if names_from_plan
                                               else parent_wgrad_name(lwv, mode, gy_ld == Cout))
            for gi, group in enumerate(GROUPS):
                descs = (ConvDesc * 3)()
                for i, (N, H, W, Cin, Cout, k, stride) in enumerate(group):
                    descs[i] = ConvDesc(N, H, W, Cin, Cout, k, k, stride, k // 2, H, W, H, W, 1, 0)
                sp, nb = (ctypes.c_int * 3)(), (ctypes.c_size_t * 3)()
                kind = lib.dadet_conv_wgrad_group_plan(descs, 3, sp, nb)
                group_cols["setting"].append(si)
                group_cols["group"].append(gi)
                group_cols["kind"].append(kind)
                group_cols["splits"].append(list(sp) if kind else [0, 0, 0])
                group_cols["bytes"].append(list(nb) if kind else [0, 0, 0])
            for k in env:
                del os.environ[k]
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
        lib.dadet_set_gemm_mode(mode0)
        lib.dadet_set_big_gemm(big0)
    out = {}
    for k, v in cols.items():
        out[k] = np.asarray(v, dtype=np.int64 if k.endswith("bytes") else np.int32)
    table = sorted(set(itertools.chain(*names.values())))
    out["names"] = np.asarray(table)
    for k, v in names.items():
        out[k] = np.asarray([table.index(n) for n in v], dtype=np.int16)
    for k, v in group_cols.items():
        out["group_" + k] = np.asarray(v, dtype=np.int64)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "conv_plans.npz"))
    ap.add_argument("--parent-names", action="store_true", help="labels derived the parent's way (recording the fixture)")
    args = ap.parse_args()
    from da_detect_amd import _lib

    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    rows = descriptors()
    out = record(_lib.load(), rows, not args.parent_names)
    out["desc"] = np.asarray(rows, dtype=np.int32)
    out["settings"] = np.asarray(json.dumps(SETTINGS))
    np.savez_compressed(args.out, **out)
    fam = out["fwd_family"][out["fwd_rc"] == 0]
    print("rows", len(out["setting"]), "bytes", os.path.getsize(args.out))
    print("forward families", {FWD_FAMILIES[f]: int((fam == f).sum()) for f in range(len(FWD_FAMILIES))})
    print("wgrad families", {WGRAD_FAMILIES[f]: int((out["wgrad_family"] == f).sum()) for f in range(len(WGRAD_FAMILIES))})


if __name__ == "__main__":
    main()
