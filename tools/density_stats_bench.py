"""Timings of the density statistics (gr_density_stats / ViewShardedFitter(density_stats=True)) on one GPU.

1. k_density_stats alone at C4's Gaussian count: batches of `--batch` views of random per-Gaussian sums, `--calls` calls
   back to back between two device events after a warm-up; the achieved bytes/s under two byte models
   (per Gaussian: 32 B x views of sums + 8 B, the statistics row; and the same plus the second 8 B of the row's
   read-modify-write and the 28 B of parameters read), as a fraction of the HBM peak (8 TB/s spec, 6.3 TB/s achievable).
   The sums of one batch are rotated over `--sets` buffers so that a call does not find its inputs in the 256 MiB
   Infinity Cache.
2. The fit step at C4 with the statistics off and on: two fitters from the same parameters, warmed up, then timed in
   alternating windows of `--steps` steps (a host clock around work that ends in a device synchronise): the median
   window and [min .. max].

    python tools/density_stats_bench.py [--gaussians 1000000 --views 50 --res 800] [--batch 4 16] [--out FILE (appended)]
"""
import argparse
import ctypes
import importlib
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
fm = importlib.import_module("3dgaussian_amd.fit_multiview")
tr = importlib.import_module("3dgaussian_amd.torch_renderer")
bench = importlib.import_module("bench")

HBM_SPEC, HBM_ACHIEVABLE = 8.0e12, 6.3e12  # bytes / s


def kernel_lines(n, batches, calls, sets, dev):
    p = bench.synthetic_params(n, dev)
    m, s, _, o = (t.detach().contiguous() for t in fm.activations(p))
    cams = fm.orbit_cameras(max(batches), 800, 800, dev)
    gvs = [tr.make_view(c.view, c.proj, 800, 800, None, cutoff=tr.FIT_CUTOFF, core_cutoff=tr.FIT_CUTOFF, depth_grad=False)
           for c in cams]
    g = torch.Generator(device=dev).manual_seed(1)
    nat = tr._native
    L = nat.lib()
    lines = []
    for nv in batches:
        pool = [[torch.randn((n, 8), generator=g, device=dev) for _ in range(nv)] for _ in range(sets)]
        stats = torch.zeros((n, 2), device=dev)
        # the C call itself on prebuilt view arrays: a few microseconds of host time per call, so the device is the limit
        arrs = []
        for q in range(sets):
            arr = (nat.GrSumsView * nv)()
            for k in range(nv):
                arr[k].view, arr[k].sums, arr[k].sums3 = gvs[k], pool[q][k].data_ptr(), None
            arrs.append(arr)
        args = (n, nat.ptr(m), nat.ptr(s), nat.ptr(o), ctypes.c_float(50.0), nat.ptr(stats),
                ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        run = lambda q: nat.check(L.gr_density_stats(nv, arrs[q % sets], *args), "gr_density_stats")
        for q in range(sets):
            run(q)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = []
        for _ in range(5):
            torch.cuda.synchronize()
            e0.record()
            for q in range(calls):
                run(q)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e-3 / calls)
        t = statistics.median(times)
        small, full = n * (32 * nv + 8), n * (32 * nv + 16 + 28)
        lines.append(f"  k_density_stats, {nv:2d} views x {n} Gaussians: {t * 1e6:8.1f} us per call [{min(times) * 1e6:.1f} .. "
                     f"{max(times) * 1e6:.1f}] (launch gaps included); {small / t / 1e12:.2f} TB/s at 32 B x views + 8 B, "
                     f"{full / t / 1e12:.2f} TB/s with the row's store and the parameters = {full / t / HBM_SPEC:.0%} of the "
                     f"8 TB/s spec, {full / t / HBM_ACHIEVABLE:.0%} of the 6.3 TB/s achievable: HBM-bound "
                     f"({nv * n * 32 * sets / 2 ** 20:.0f} MiB of sums in rotation)")
        del pool
    return lines


def window_ms(fit, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fit.step()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def step_lines(n, views, R, steps, windows, warmup, dev):
    cams = fm.orbit_cameras(views, R, R, dev)
    g = torch.Generator(device=dev).manual_seed(3)
    targets = [torch.rand((R, R, 3), generator=g, device=dev) for _ in cams]
    masks = [(t.mean(dim=2) > 0.5).float() for t in targets]
    fits = {}
    for name, on in (("off", False), ("on", True)):
        fits[name] = fm.ViewShardedFitter(bench.synthetic_params(n, dev), cams, targets, R, R, masks=masks, density_stats=on)
        for _ in range(warmup):
            fits[name].step()
    times = {k: [] for k in fits}
    for _ in range(windows):
        for k, f in fits.items():
            times[k].append(window_ms(f, steps))
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = [f"  fit step, {n} Gaussians, {views} views {R}x{R}: {windows} alternating windows of {steps} steps after {warmup} "
             "warm-up steps, median ms per step [min .. max]"]
    for k in fits:
        lines.append(f"    density_stats {k:3s}: {med[k]:9.3f} ms  [{min(times[k]):.3f} .. {max(times[k]):.3f}]")
    lines.append(f"    on / off: {med['on'] / med['off']:.4f}")
    gsum, seen = fits["on"].density_state()
    lines.append(f"    after {warmup + windows * steps} steps: {int((seen > 0).sum())} of {n} Gaussians seen, "
                 f"mean seeing views per step {float(seen.sum()) / n / (warmup + windows * steps):.1f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--views", type=int, default=50)
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--batch", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--calls", type=int, default=64)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("density_stats_bench: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda", 0)
    lines = [f"density statistics on {torch.cuda.get_device_name(0)}"]
    lines += kernel_lines(args.gaussians, args.batch, args.calls, args.sets, dev)
    lines += step_lines(args.gaussians, args.views, args.res, args.steps, args.windows, args.warmup, dev)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
