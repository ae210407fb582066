"""The fused D-SSIM loss (losses.dssim_loss: gr_ssim_fwd + gr_ssim_bwd) against the torch conv2d composition it
replaces, forward + backward at one image size on one GPU, and the kernels' gradient error per test shape.

Timing: both versions are warmed up, then timed in alternating windows of `iters` iterations between HIP events
(the median window counts); the ABI calls are also timed alone on preallocated buffers (no autograd, no allocator).
Byte model of the fused op: the forward reads 2 images and writes 3 maps, the backward reads 3 maps and 2 images and
writes 1: 11 floats per value; the achieved rate is given as a fraction of the 8 TB/s HBM peak.
Errors: max|g - g_ref| / max|g_ref| against the float64 dense-window reference of tests/ssim_reference.py, beside
the float32 dense torch evaluation's (e32), whose 4-fold is the tests' bound.

    python tools/ssim_bench.py [--res 800] [--channels 3] [--iters 50] [--windows 5] [--out profiles/ssim_loss.txt]
"""
import argparse
import ctypes
import importlib
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
losses = importlib.import_module("3dgaussian_amd.losses")
nat = importlib.import_module("3dgaussian_amd._native")
sr = importlib.import_module("ssim_reference")

HBM_PEAK = 8.0e12  # bytes / s


def window_ms(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ssim_loss.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ssim_bench: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda", 0)
    H = W = args.res
    C = args.channels
    gen = torch.Generator().manual_seed(0)
    x = torch.rand((H, W, C), generator=gen).to(dev)
    y = torch.rand((H, W, C), generator=gen).to(dev)
    pred = x.clone().requires_grad_(True)

    def fused():
        (g,) = torch.autograd.grad(losses.dssim_loss(pred, y), pred)
        return g

    def composed():
        (g,) = torch.autograd.grad(1.0 - losses._ssim_mean_torch(pred, y), pred)
        return g

    L = nat.lib()
    need = int(L.gr_ssim_ws_bytes(H, W, C, 1))
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    out, one, gx = torch.empty((), device=dev), torch.ones((), device=dev), torch.empty_like(x)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def abi():
        nat.check(L.gr_ssim_fwd(nat.ptr(x), nat.ptr(y), H, W, C, 1, nat.ptr(out), nat.ptr(ws), need, stream), "gr_ssim_fwd")
        nat.check(L.gr_ssim_bwd(nat.ptr(x), nat.ptr(y), H, W, C, nat.ptr(one), nat.ptr(ws), need, nat.ptr(gx), stream),
                  "gr_ssim_bwd")

    def abi_fwd():
        nat.check(L.gr_ssim_fwd(nat.ptr(x), nat.ptr(y), H, W, C, 1, nat.ptr(out), nat.ptr(ws), need, stream), "gr_ssim_fwd")

    fns = {"fused dssim_loss (autograd, fwd+bwd)": fused, "torch conv2d composition (autograd, fwd+bwd)": composed,
           "gr_ssim_fwd + gr_ssim_bwd alone": abi, "gr_ssim_fwd alone (with maps)": abi_fwd}
    for fn in fns.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    agree = float((fused() - composed()).abs().max() / composed().abs().max())
    times = {k: [] for k in fns}
    for _ in range(args.windows):  # alternating windows
        for k, fn in fns.items():
            times[k].append(window_ms(fn, args.iters))
    med = {k: statistics.median(v) for k, v in times.items()}

    lines = [f"D-SSIM loss, {torch.cuda.get_device_name(0)}, {H}x{W}x{C} float32, forward + backward",
             f"(tools/ssim_bench.py: {args.windows} alternating windows of {args.iters} iterations after {args.warmup} warm-up "
             "iterations each, HIP events; median window, [min .. max])", ""]
    for k in fns:
        lines.append(f"  {k:48s} {1e3 * med[k]:9.1f} us  [{1e3 * min(times[k]):.1f} .. {1e3 * max(times[k]):.1f}]")
    a, b = "fused dssim_loss (autograd, fwd+bwd)", "torch conv2d composition (autograd, fwd+bwd)"
    lines.append(f"  fused / composition: {med[a] / med[b]:.3f} (speed-up {med[b] / med[a]:.1f}x); "
                 f"max|g_fused - g_composed| / max|g| = {agree:.2e}")
    n = H * W * C
    t_all, t_fwd = med["gr_ssim_fwd + gr_ssim_bwd alone"], med["gr_ssim_fwd alone (with maps)"]
    lines.append(f"  byte model: forward {5 * 4 * n / 1e6:.1f} MB, backward {6 * 4 * n / 1e6:.1f} MB; the calls alone move "
                 f"{11 * 4 * n / (t_all * 1e-3) / 1e12:.2f} TB/s = {11 * 4 * n / (t_all * 1e-3) / HBM_PEAK:.1%} of the HBM peak "
                 f"(forward {5 * 4 * n / (t_fwd * 1e-3) / HBM_PEAK:.1%}, backward "
                 f"{6 * 4 * n / (max(t_all - t_fwd, 1e-9) * 1e-3) / HBM_PEAK:.1%}); times include the launch gaps")
    lines += ["", "Gradient error of the kernels per test shape (of 3 * loss; tests/test_ssim_gpu.py::test_gradient):",
              f"  {'input':8s} {'shape':12s} {'err/max|g|':>11s} {'e32/max|g|':>11s} {'bound/max|g|':>13s} {'value err':>10s}"]
    for kind in sr.KINDS:
        for shape in sr.SHAPES:
            xs, ys = (t.to(dev) for t in sr.inputs(kind, shape))
            ref = sr.reference(kind, shape)
            p = xs.clone().requires_grad_(True)
            loss = losses.dssim_loss(p, ys)
            (g,) = torch.autograd.grad(sr.GRAD_SCALE * loss, p)
            err = float((g.double().cpu() - ref["grad"]).abs().max())
            lines.append(f"  {kind:8s} {'x'.join(map(str, shape)):12s} {err / ref['gmax']:11.2e} {ref['e32'] / ref['gmax']:11.2e} "
                         f"{sr.grad_bound(ref) / ref['gmax']:13.2e} {abs(float(loss.detach()) - ref['loss']):10.2e}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
