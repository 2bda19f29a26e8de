"""A/B harness: tile configurations (ids of tuning key 0: k_conv_igemm and, from 100 on, k_gemm_stream) interleaved in rounds inside one
process, median over rounds.

    python scratch/conv_sweep.py CFG[,CFG...] [SHAPE[,SHAPE...] [ROUNDS]]
"""
import sys, os
sys.path[:0] = [os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tf-faster-rcnn_amd")]
import numpy as np, torch
from frcnn_hip import ops, lib
dev = torch.device("cuda:0")
L = lib()
shapes = {  # name: (N,H,W,Cin,Cout,k,pad)
 "b3c1": (1,38,63,1024,256,1,0), "b3c2": (1,38,63,256,256,3,1), "b3c3": (1,38,63,256,1024,1,0),
 "rpn":  (1,38,63,1024,512,3,1), "b2c2": (1,75,125,128,128,3,1), "b2c3": (1,75,125,128,512,1,0), "b2c1": (1,75,125,512,128,1,0),
 "b1c2": (1,150,250,64,64,3,1), "b1c3": (1,150,250,64,256,1,0),
 "b3c1x4": (4,38,63,1024,256,1,0), "b3c2x4": (4,38,63,256,256,3,1), "b3c3x4": (4,38,63,256,1024,1,0), "rpnx4": (4,38,63,1024,512,3,1),
 "b2c2x4": (4,75,125,128,128,3,1), "b2c3x4": (4,75,125,128,512,1,0), "b2c1x4": (4,75,125,512,128,1,0), "b1c2x4": (4,150,250,64,64,3,1),
 "b1c3x4": (4,150,250,64,256,1,0), "b1c1x4": (4,150,250,256,64,1,0),
 "b4c1x4": (1200,7,7,2048,512,1,0), "b4c3x4": (1200,7,7,512,2048,1,0),
 "b4c1": (300,7,7,2048,512,1,0), "b4c2": (300,7,7,512,512,3,1), "b4c3": (300,7,7,512,2048,1,0),
}
cfgs = [int(c) for c in sys.argv[1].split(",")]
only = sys.argv[2].split(",") if len(sys.argv) > 2 else list(shapes)
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5


def tune(key, value):
    rc = L.frcnn_set_tuning(key, value)
    if rc:
        raise SystemExit("frcnn_set_tuning(%d, %d) returned %d" % (key, value, rc))


print("%-6s %4s %9s %9s %8s" % ("shape", "cfg", "med_us", "min_us", "TFLOP/s"))
for name in only:
    N,H,W,Cin,Cout,k,pad = shapes[name]
    x = torch.randn(N,H,W,Cin, device=dev); w = torch.randn(Cout,k,k,Cin, device=dev) * 0.05; b = torch.randn(Cout, device=dev)
    res = torch.randn(N,H,W,Cout, device=dev) if name.endswith("c3") else None
    out = torch.empty(N,H,W,Cout, device=dev)
    flops = 2.0*N*H*W*Cout*k*k*Cin
    times = {c: [] for c in cfgs}
    for r in range(rounds + 1):
        for cfg in cfgs:
            tune(0, cfg)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(8): ops.conv2d(x, w, b, k, k, 1, (pad,)*4, 1, res, 1, out=out)      # raises when the launch reports an error
            e1.record(); torch.cuda.synchronize()
            if r: times[cfg].append(e0.elapsed_time(e1) * 1000 / 8)
    for cfg, ts in times.items():
        med = float(np.median(ts))
        print("%-6s %4d %9.1f %9.1f %8.1f" % (name, cfg, med, min(ts), flops / med / 1e6))
tune(0, -1)
