"""Times the per-tensor parameter update at the C4 tensor sizes (1M Gaussians: means and scales 3M floats, opacities 1M, SH
48M): gr_fit_param_step with and without Adam (four stream accumulators) and gr_adam_step, HIP events around 50 calls after 5
warm-ups.  One JSON line of microseconds per call; GR_HIP_LIB selects the library.   python tools/param_step_bench.py"""
import ctypes
import importlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
nat = importlib.import_module("3dgaussian_amd")._native
L = nat.lib()
cuda = torch.device("cuda:0")
stream = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
B1, B2, EPS, NEG_STEP, BC2S = 0.9, 0.999, 1e-15, -1e-3, 0.5
out = {}
for name, n, act in (("means", 3_000_000, 0), ("scales", 3_000_000, 1), ("opacities", 1_000_000, 2), ("sh", 48_000_000, 0)):
    p, g, m = torch.randn(n, device=cuda), torch.empty(n, device=cuda), torch.zeros(n, device=cuda)
    v = torch.zeros(n, device=cuda)
    accs = [torch.randn(n, device=cuda) * 1e-3 for _ in range(4)]
    ptrs = (ctypes.c_void_p * 4)(*[x.data_ptr() for x in accs])
    calls = {
        "step_adam": lambda: L.gr_fit_param_step(n, act, nat.ptr(p), nat.ptr(g), ptrs, 4, 1e-6, 1, nat.ptr(m), nat.ptr(v),
                                                 NEG_STEP, BC2S, B1, B2, EPS, stream),
        "step_grad": lambda: L.gr_fit_param_step(n, act, nat.ptr(p), nat.ptr(g), ptrs, 4, 1e-6, 0, None, None, NEG_STEP,
                                                 BC2S, B1, B2, EPS, stream),
        "adam": lambda: L.gr_adam_step(n, nat.ptr(p), nat.ptr(g), nat.ptr(m), nat.ptr(v), NEG_STEP, BC2S, B1, B2, EPS, stream),
    }
    for what, call in calls.items():
        for _ in range(5):
            nat.check(call(), what)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(50):
            nat.check(call(), what)
        t1.record()
        torch.cuda.synchronize()
        out[f"{name}.{what}"] = round(t0.elapsed_time(t1) * 1000.0 / 50, 2)
print(json.dumps(out))
