"""ms per fit step of a D-SSIM fit (ViewShardedFitter, dssim_weight > 0) with dssim_fused off (the per-view autograd
path: drop-in op, l1_loss + dssim_loss, a gradient image, gr_bwd) and on (the fused path's D-SSIM form:
gr_fwd_render + gr_bwd_fit_ssim_gather per view, batched gr_reduce_sums, the fused parameter step), one GPU.

Both fitters start from the same synthetic parameters and are warmed up; then they are timed in alternating windows of
`steps` steps, a host clock around work that ends in a device synchronise.  Reported: the median window, [min .. max]
over the windows, and the first-step losses of the two paths (they minimise the same objective).

    python tools/dssim_fused_bench.py [--gaussians 1000000 --views 50 --res 800] [--lam 0.2] [--steps 5] [--windows 5]
                                      [--label C4] [--out FILE (appended)]
"""
import argparse
import importlib
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
fm = importlib.import_module("3dgaussian_amd.fit_multiview")
bench = importlib.import_module("bench")


def window_ms(fit, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fit.step()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--views", type=int, default=50)
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--lam", type=float, default=0.2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dssim_fused_bench: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda", 0)
    R = args.res
    cams = fm.orbit_cameras(args.views, R, R, dev)
    g = torch.Generator(device=dev).manual_seed(3)
    targets = [torch.rand((R, R, 3), generator=g, device=dev) for _ in cams]
    masks = [(t.mean(dim=2) > 0.5).float() for t in targets]
    fits, first = {}, {}
    for name, fused in (("unfused", False), ("fused", True)):
        fits[name] = fm.ViewShardedFitter(bench.synthetic_params(args.gaussians, dev), cams, targets, R, R, masks=masks,
                                          dssim_weight=args.lam, dssim_fused=fused)
        first[name] = float(fits[name].step())
        for _ in range(max(0, args.warmup - 1)):
            fits[name].step()
    times = {k: [] for k in fits}
    for _ in range(args.windows):  # alternating windows
        for k, f in fits.items():
            times[k].append(window_ms(f, args.steps))
    med = {k: statistics.median(v) for k, v in times.items()}
    head = (f"{args.label + ': ' if args.label else ''}{args.gaussians} Gaussians, {args.views} views, {R}x{R}, l = {args.lam}, "
            f"{torch.cuda.get_device_name(0)}; {args.windows} alternating windows of {args.steps} steps after {args.warmup} "
            "warm-up steps, median ms per step [min .. max]")
    lines = [head]
    for k in fits:
        lines.append(f"  dssim_fused {'on ' if k == 'fused' else 'off'}: {med[k]:9.3f} ms  [{min(times[k]):.3f} .. {max(times[k]):.3f}]"
                     f"  first-step loss {first[k]:.6f}")
    lines.append(f"  fused / unfused: {med['fused'] / med['unfused']:.3f} (speed-up {med['unfused'] / med['fused']:.2f}x)")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
