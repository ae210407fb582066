"""Timings of the camera gradients of the fused fit path (gr_camera_grads_sums / ViewShardedFitter(refine_cameras=True))
on one GPU.

1. k_camera_grad_views + k_camera_final_views alone at C4's Gaussian count: batches of `--batch` views of random
   per-Gaussian sums, `--calls` calls back to back between two device events after a warm-up; the achieved bytes/s under
   the byte model 32 B x views of sums + the parameter bytes (means 12, scales 12, opacity 4, colours 4 x colour dim)
   per Gaussian, as a fraction of the HBM peak (8 TB/s spec, 6.3 TB/s achievable).  The sums of one batch are rotated
   over `--sets` buffers so that a call does not find its inputs in the 256 MiB Infinity Cache.  `--kernel-only` runs
   this part alone (for a kernel trace in a run of its own: rocprofv3 --kernel-trace --stats -- python tools/... ).
2. The fit step at C4 with refinement off and on: two fitters from the same parameters, warmed up, then timed in
   alternating windows of `--steps` steps (a host clock around work that ends in a device synchronise): the median
   window and [min .. max].  `--step-only off` times the off side alone and prints its losses as hex floats (the same
   file runs in a checkout of the parent commit, whose fitter has no refine_cameras argument: off against the parent).

    python tools/camera_refine_bench.py [--gaussians 1000000 --views 50 --res 800] [--batch 4 16] [--out FILE (appended)]
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
    m, s, c, o = (t.detach().contiguous() for t in fm.activations(p))
    cd = tr._color_dim(c)
    cams = fm.orbit_cameras(max(batches), 800, 800, dev)
    gvs = [tr.make_view(cam.view, cam.proj, 800, 800, None, cutoff=tr.FIT_CUTOFF, core_cutoff=tr.FIT_CUTOFF, depth_grad=False)
           for cam in cams]
    g = torch.Generator(device=dev).manual_seed(1)
    nat = tr._native
    L = nat.lib()
    lines = []
    for nv in batches:
        pool = [[torch.randn((n, 8), generator=g, device=dev) for _ in range(nv)] for _ in range(sets)]
        rows = torch.zeros((nv, nat.CAMERA_GRADS), device=dev)
        out = (ctypes.c_void_p * nv)(*[rows[k].data_ptr() for k in range(nv)])
        ws = torch.empty((int(L.gr_camera_grads_ws_bytes(n, nv)),), dtype=torch.uint8, device=dev)
        # the C call itself on prebuilt view arrays: a few microseconds of host time per call, so the device is the limit
        arrs = []
        for q in range(sets):
            arr = (nat.GrSumsView * nv)()
            for k in range(nv):
                arr[k].view, arr[k].sums, arr[k].sums3 = gvs[k], pool[q][k].data_ptr(), None
            arrs.append(arr)
        args = (n, nat.ptr(m), nat.ptr(s), nat.ptr(c), cd, nat.ptr(o), out, nat.ptr(ws), ws.numel(),
                ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        run = lambda q: nat.check(L.gr_camera_grads_sums(nv, arrs[q % sets], *args), "gr_camera_grads_sums")
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
        model = n * (32 * nv + 28 + 4 * cd)
        lines.append(f"  gr_camera_grads_sums (k_camera_grad_views + k_camera_final_views), {nv:2d} views x {n} Gaussians, colour "
                     f"dim {cd}: {t * 1e6:8.1f} us per call [{min(times) * 1e6:.1f} .. {max(times) * 1e6:.1f}] (launch gaps "
                     f"included); {model / t / 1e12:.2f} TB/s at 32 B x views + {28 + 4 * cd} B = {model / t / HBM_SPEC:.0%} of "
                     f"the 8 TB/s spec, {model / t / HBM_ACHIEVABLE:.0%} of the 6.3 TB/s achievable "
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


def step_lines(n, views, R, steps, windows, warmup, dev, sides):
    cams = fm.orbit_cameras(views, R, R, dev)
    g = torch.Generator(device=dev).manual_seed(3)
    targets = [torch.rand((R, R, 3), generator=g, device=dev) for _ in cams]
    masks = [(t.mean(dim=2) > 0.5).float() for t in targets]
    fits, first = {}, {}
    for name in sides:
        kw = {"refine_cameras": True} if name == "on" else {}  # (off: no argument, as a fitter of the parent commit)
        fits[name] = fm.ViewShardedFitter(bench.synthetic_params(n, dev), cams, targets, R, R, masks=masks, **kw)
        first[name] = [float(fits[name].step()) for _ in range(warmup)]
    times = {k: [] for k in fits}
    for _ in range(windows):
        for k, f in fits.items():
            times[k].append(window_ms(f, steps))
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = [f"  fit step, {n} Gaussians, {views} views {R}x{R}, {fm.NUM_STREAMS} streams: {windows} alternating windows of "
             f"{steps} steps after {warmup} warm-up steps, median ms per step [min .. max]"]
    for k in fits:
        lines.append(f"    refine_cameras {k:3s}: {med[k]:9.3f} ms  [{min(times[k]):.3f} .. {max(times[k]):.3f}]")
        lines.append(f"      losses of the warm-up steps: {' '.join(v.hex() for v in first[k])}")
    if "on" in fits and "off" in fits:
        lines.append(f"    on / off: {med['on'] / med['off']:.4f}")
    if "on" in fits:
        xi, grad = fits["on"].camera_state()
        lines.append(f"    after {warmup + windows * steps} steps: largest pose delta {float(xi.abs().max()):.3e}, "
                     f"|d loss / d xi| {float(grad.norm()):.3e}")
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
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--step-only", choices=("off", "both"), default="")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("camera_refine_bench: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda", 0)
    lines = [f"camera refinement on {torch.cuda.get_device_name(0)}" + (f" ({args.label})" if args.label else "")]
    if not args.step_only:
        lines += kernel_lines(args.gaussians, args.batch, args.calls, args.sets, dev)
    if not args.kernel_only:
        sides = ("off",) if args.step_only == "off" else ("off", "on")
        lines += step_lines(args.gaussians, args.views, args.res, args.steps, args.windows, args.warmup, dev, sides)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
