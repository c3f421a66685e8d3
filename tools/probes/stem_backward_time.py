"""launch times of the trainable stem's backward (MODEL.BACKBONE.FREEZE_CONV_BODY_AT 0) at the workload's size, a
[2,64,512,1024] stem activation: the max-pool backward fused with the ReLU gate and the FrozenBN scale, next to
relu_bn_backward on a tensor of the same size (the streaming kernel of the same traffic class), and the weight-gradient
launch of the padded [64,4,7,8] kernel against its HBM bound.  Events around 20 launches after 5 warm-up launches."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from da_detect_amd import _C  # noqa: E402

CL = torch.channels_last
dev = torch.device("cuda", 0)
N, C, H, W = 2, 64, 512, 1024
Ho, Wo = H // 2, W // 2


def timed(fn, warmup=5, launches=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches      # ms per launch


def report(name, ms, nbytes):
    print("%-44s %8.1f us  %7.1f MB  %6.2f TB/s" % (name, ms * 1e3, nbytes / 1e6, nbytes / ms / 1e9))
    return ms / nbytes


torch.manual_seed(0)
image = torch.randn((N, 3, 2 * H, 2 * W), device=dev) * 50.0
x4 = _C.nchw3_to_nhwc4(image)
y = torch.relu(torch.randn((N, C, H, W), device=dev)).contiguous(memory_format=CL)
gp = torch.randn((N, C, Ho, Wo), device=dev).contiguous(memory_format=CL)
gfull = torch.randn((N, C, H, W), device=dev).contiguous(memory_format=CL)
scale = torch.rand(C, device=dev) + 0.5
print("contraction mode %d; stem activation %s (half of its values zero, like a ReLU output)" % (
    _C.get_gemm_mode(), tuple(y.shape)))

act = 4.0 * y.numel()
pool = report("maxpool3x3s2_relu_backward (y, gp in; g out)", timed(lambda: _C.maxpool3x3s2_relu_backward(y, gp, scale)),
              2 * act + 4.0 * gp.numel())
gate = report("relu_bn_backward (g, y in; g_scaled out)", timed(lambda: _C.relu_bn_backward(gfull, y, scale)), 3 * act)
print("time per algorithmic byte: pool backward / relu_bn_backward = %.2f" % (pool / gate))

g = _C.maxpool3x3s2_relu_backward(y, gp, scale)
ms = timed(lambda: _C.conv_wgrad(x4, g, (64, 4, 7, 8), stride=2, pad=3))
nbytes = 4.0 * (g.numel() + x4.numel())
report("conv_wgrad [64,4,7,8] s2 (g, x4 in; + reduce)", ms, nbytes)
print("HBM bound of that launch at 6.3 TB/s: %.1f us; its %d x %d x %d GEMM: %.1f TFLOP/s" % (
    nbytes / 6.3e12 * 1e6, N * H * W, 64, 224, 2.0 * N * H * W * 64 * 224 / ms / 1e9))
