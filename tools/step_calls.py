#!/usr/bin/env python
"""One line per native call of one training step, in the order the step makes them.

The recipe is built as tests/test_default_path_gpu.py builds it (seeded weights, the synthetic batch of the seed, the
overlapped RPN backward, one train_step).  A line is the entry's name; where the call's first argument is a convolution
descriptor (or an array of them) the descriptor's static fields follow: Cin Cout KH KW stride pad relu_mode.  Row counts
depend on the data and are left out, so two trees that schedule the step alike print the same text:

    python tools/step_calls.py --case da_plain --hw 192x320 > a.txt        # in each tree, then diff a.txt b.txt
"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
STATIC = ("Cin", "Cout", "KH", "KW", "stride", "pad", "relu_mode")


def _descs(arg):
    from da_detect_amd._lib import ConvDesc
    arg = getattr(arg, "_obj", arg)                     # ctypes.byref(desc)
    if isinstance(arg, ConvDesc):
        return [arg]
    return list(arg) if isinstance(arg, ctypes.Array) and arg._type_ is ConvDesc else []


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--case", default="da_plain", choices=("da_plain", "da_img_only", "da_triplet_aligned", "fpn_dcn_da"))
    ap.add_argument("--hw", default="192x320")
    ap.add_argument("--k", type=int, default=1, choices=(1, 2), help="images per domain")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    H, W = (int(v) for v in args.hw.split("x"))

    import torch
    from da_detect_amd import _lib
    from da_detect_amd.data.synthetic import make_batch
    from da_detect_amd.engine.trainer import enable_overlapped_rpn_backward, train_step
    from da_detect_amd.modeling.detector import build_detection_model
    from da_detect_amd.parallel.reducer import BucketedGradReducer
    from da_detect_amd.solver import make_optimizer
    from golden.cases import case_cfg, fpn_dcn_da_cfg
    from golden.fill import fill_state_dict

    dev = torch.device("cuda:0")
    c = fpn_dcn_da_cfg() if args.case == "fpn_dcn_da" else case_cfg(args.case)
    model = build_detection_model(c)
    sd = fill_state_dict(model.state_dict(), args.seed)
    for key in sd:
        if ".conv2.offset." in key:
            sd[key] = sd[key] * 0.05
    model.load_state_dict(sd)
    model = model.to(dev).train()
    domains = 3 if c.MODEL.DA_HEADS.TRIPLET_USE else 2
    images, targets = make_batch(c, domains * args.k, H, W, seed=args.seed, device=dev, num_source=args.k)
    opt = make_optimizer(c, model)
    opt.attach_reducer(BucketedGradReducer([p for p in model.parameters() if p.requires_grad]))
    enable_overlapped_rpn_backward(model)

    native = _lib.call

    def call(name, *a):
        print(" ".join([name] + [" ".join(str(getattr(d, f)) for f in STATIC) for d in _descs(a[0] if a else None)]))
        return native(name, *a)

    _lib.call = call
    train_step(model, opt, images, targets)
    torch.cuda.synchronize()
    _lib.call = native


if __name__ == "__main__":
    main()
