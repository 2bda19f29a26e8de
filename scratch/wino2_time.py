"""Isolated timing at the bench shape 8 x 150 x 250 x 64: the fused launch against the three launches of the parent route, alternating."""
import os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))      # python scratch/wino2_time.py
sys.path.insert(0, os.path.join(ROOT, "tf-faster-rcnn_amd")); sys.path.insert(0, os.path.join(ROOT, "tf-faster-rcnn_amd", "lib"))
import torch
from frcnn_hip import ops
dev = torch.device("cuda:0")
N, H, W, C = 8, 150, 250, 64
g = torch.Generator(device=dev); g.manual_seed(1)
x = (torch.randn(N, H, W, C, device=dev, generator=g).clamp_(min=0) * torch.exp(torch.rand(N, H, W, 1, device=dev, generator=g) * 4 - 2)).contiguous()
w = (torch.randn(3, 3, C, C, device=dev, generator=g) / 24).cpu().numpy()
u = torch.from_numpy(ops.winograd_filter_transform(w, m=2)).to(dev)
planes = ops.gemm_x3_pack(u)
b = torch.randn(C, device=dev, generator=g)
T = ops.winograd_tiles(N, H, W, 2)
v = torch.empty(16, T, C, device=dev); mm = torch.empty(16, T, C, device=dev)
y0 = torch.empty(N, H, W, C, device=dev); y1 = torch.empty(N, H, W, C, device=dev)
def ev(): return torch.cuda.Event(enable_timing=True)
def timed(fn):
    a, z = ev(), ev(); a.record(); fn(); z.record(); return a, z
R = {"fused": [], "wino_in": [], "gemm_x3": [], "wino_out": []}
for it in range(60):
    e = {}
    e["wino_in"] = timed(lambda: ops.winograd_input_transform(x, v, 2))
    e["gemm_x3"] = timed(lambda: ops.gemm_x3(v, planes, 16, T, C, C, out=mm))
    e["wino_out"] = timed(lambda: ops.winograd_output_transform(mm, b, 1, y0, 2))
    e["fused"] = timed(lambda: ops.winograd2_conv_x3(x, planes, b, 1, y1))
    torch.cuda.synchronize()
    if it >= 10:
        for k, (a, z) in e.items(): R[k].append(a.elapsed_time(z) * 1000.0)
print("bit equal at the bench shape:", torch.equal(y0.view(torch.int32), y1.view(torch.int32)))
for k in ("wino_in", "gemm_x3", "wino_out", "fused"):
    print("%-9s median %7.1f us   min %7.1f us   (n = %d)" % (k, statistics.median(R[k]), min(R[k]), len(R[k])))
print("three launches: median sum %.1f us" % sum(statistics.median(R[k]) for k in ("wino_in", "gemm_x3", "wino_out")))
