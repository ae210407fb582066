"""What per-pixel loss weights cost on the HIP device (ViewShardedFitter(weights=...): the fused path's weighted form,
gr_fwd_render + gr_bwd_fit_weighted_gather per view, the Python schedule), one GPU.

1. default: ms per fit step of four fitters from the same synthetic parameters on the same targets:
     l1          no weights, no depth term: the L1 form (gr_fwd_render_l1's epilogue, FIT_TILE tiles, every schedule)
     weighted    the same fit with weights: the sums route (saved sums + the gather entry, 16-pixel tiles)
     depth       no weights, with a depth term: the depth form (gr_fwd_render + gr_bwd_fit_gather), Python schedule
     weighted+d  the same fit with weights: gr_bwd_fit_weighted_gather in gr_bwd_fit_gather's place
   The pair depth / weighted+d runs the same views through the same schedule and differs in the upstream kernel and the
   depth loss's tile sums only; l1 / weighted also pays the sums route against the L1 form's fused epilogue.  All are
   warmed up, then timed in alternating windows of `steps` steps, a host clock around work that ends in a device
   synchronise.  Reported: the median window and [min .. max].  --plain-only: the two fitters without weights only
   (what an older tree's fitter can run: the same session's figure of the parent commit).
2. --kernel-loop N: one view's saved sums without and one with a depth gradient, then N calls each of
   gr_bwd_fit_gather, gr_bwd_fit_exposure_gather and gr_bwd_fit_weighted_gather on the first and of gr_bwd_fit_gather
   and gr_bwd_fit_weighted_gather with a depth target on the second, alternating, each between device events (the
   entry's time: upstream kernels + splat + gather).  For the kernels' own times run it under a kernel trace in a run of
   its own (rocprofv3 --kernel-trace --stats -- python tools/weights_bench.py --kernel-loop 50; tools/kstats.py):
   k_pixel_grads_wgt beside k_pixel_grads and k_pixel_grads_expo, k_depth_tile_sums_wgt beside k_depth_tile_sums.

    python tools/weights_bench.py [--gaussians 1000000 --views 50 --res 800] [--steps 5] [--windows 5] [--label C4]
                                  [--kernel-loop N] [--plain-only] [--out FILE (appended)]
Run it under `timeout`.
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
tr = importlib.import_module("3dgaussian_amd.torch_renderer")
bench = importlib.import_module("bench")


def window_ms(fit, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fit.step()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def emit(text, out):
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(text)


def weight_map(R, g, dev):
    """Random weights in [0.25, 4] with a rectangle of zeros over about a quarter of the pixels."""
    w = 0.25 + 3.75 * torch.rand((R, R), generator=g, device=dev)
    w[R // 4:3 * R // 4, R // 4:3 * R // 4] = 0.0
    return w.contiguous()


def kernel_loop(args, dev):
    R = args.res
    p = bench.synthetic_params(args.gaussians, dev)
    m, s, c, o = (t.detach().contiguous() for t in fm.activations(p))
    cam = fm.orbit_cameras(args.views, R, R, dev)[1]
    g = torch.Generator(device=dev).manual_seed(3)
    target = torch.rand((R, R, 3), generator=g, device=dev)
    mask = (target.mean(dim=2) > 0.5).float()
    tdepth = torch.rand((R, R), generator=g, device=dev)
    w = weight_map(R, g, dev)
    gv = tr.make_view(cam.view, cam.proj, R, R, None, cutoff=tr.FIT_CUTOFF, core_cutoff=tr.FIT_CUTOFF, depth_grad=False)
    _, _, _, st = tr.forward_native(m, s, c, o, gv, images=False)
    gvd = tr.make_view(cam.view, cam.proj, R, R, None, depth_grad=True)
    _, _, _, std = tr.forward_native(m, s, c, o, gvd, images=False)
    E = torch.tensor([1.1, 0.02, -0.01, 0.03, 0.01, 0.9, 0.02, -0.02, -0.02, 0.01, 1.05, 0.01], device=dev)
    dE, loss = torch.zeros(12, device=dev), torch.zeros(1, device=dev)
    calls = {
        "gr_bwd_fit_gather": lambda: tr.backward_fit_gather_native(st, target, mask, 0.2, None, 0.0, 0.02, loss),
        "gr_bwd_fit_exposure_gather": lambda: tr.backward_fit_exposure_gather_native(st, target, mask, 0.2, None, 0.0, 0.02,
                                                                                     E, dE, loss),
        "gr_bwd_fit_weighted_gather": lambda: tr.backward_fit_weighted_gather_native(st, target, mask, 0.2, None, 0.0, 0.02,
                                                                                     w, loss),
        "gr_bwd_fit_gather, depth": lambda: tr.backward_fit_gather_native(std, target, mask, 0.2, tdepth, 0.05, 0.02, loss),
        "gr_bwd_fit_weighted_gather, depth": lambda: tr.backward_fit_weighted_gather_native(std, target, mask, 0.2, tdepth,
                                                                                            0.05, 0.02, w, loss),
    }
    times = {k: [] for k in calls}
    for it in range(args.kernel_loop + 3):
        for k, fn in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if it >= 3:  # (three warm-up rounds)
                times[k].append(1e3 * a.elapsed_time(b))
    lines = [f"{args.label + ': ' if args.label else ''}one view {R}x{R}, {args.gaussians} Gaussians, {st.num_pairs} pairs "
             f"(with a depth gradient {std.num_pairs}), {torch.cuda.get_device_name(0)}; {args.kernel_loop} alternating calls "
             "after 3 warm-up rounds, device events around each entry (upstream kernels + backward splat + gather), median us "
             "[min .. max]"]
    for k, v in times.items():
        lines.append(f"  {k:34s} {statistics.median(v):9.1f} us  [{min(v):.1f} .. {max(v):.1f}]")
    emit("\n".join(lines) + "\n", args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--views", type=int, default=50)
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-loop", type=int, default=0)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("weights_bench: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda", 0)
    if args.kernel_loop > 0:
        return kernel_loop(args, dev)
    R = args.res
    cams = fm.orbit_cameras(args.views, R, R, dev)
    g = torch.Generator(device=dev).manual_seed(3)
    targets = [torch.rand((R, R, 3), generator=g, device=dev) for _ in cams]
    masks = [(t.mean(dim=2) > 0.5).float() for t in targets]
    depths = [torch.rand((R, R), generator=g, device=dev) for _ in cams]
    kinds = [("l1", None, {}), ("depth", depths, {})]
    if not args.plain_only:
        wgt = dict(weights=[weight_map(R, g, dev) for _ in cams])
        kinds = [("l1", None, {}), ("weighted", None, wgt), ("depth", depths, {}), ("weighted+d", depths, wgt)]
    fits, first, forms = {}, {}, {}
    for name, dep, kw in kinds:
        fits[name] = fm.ViewShardedFitter(bench.synthetic_params(args.gaussians, dev), cams, targets, R, R, masks=masks,
                                          depths=dep, **kw)
        forms[name] = fits[name]._form()
        first[name] = float(fits[name].step())
        for _ in range(max(0, args.warmup - 1)):
            fits[name].step()
    times = {k: [] for k in fits}
    for _ in range(args.windows):  # alternating windows
        for k, f in fits.items():
            times[k].append(window_ms(f, args.steps))
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = [f"{args.label + ': ' if args.label else ''}{args.gaussians} Gaussians, {args.views} views, {R}x{R}, "
             f"{torch.cuda.get_device_name(0)}; {args.windows} alternating windows of {args.steps} steps after {args.warmup} "
             "warm-up steps, median ms per step [min .. max]"]
    for k in fits:
        lines.append(f"  {k:11s} (form {forms[k]:8s}): {med[k]:9.3f} ms  [{min(times[k]):.3f} .. {max(times[k]):.3f}]"
                     f"  first-step loss {first[k]:.6f}")
    if not args.plain_only:
        lines.append(f"  weighted+d / depth: {med['weighted+d'] / med['depth']:.3f}   weighted / l1: {med['weighted'] / med['l1']:.3f}")
    emit("\n".join(lines) + "\n", args.out)


if __name__ == "__main__":
    main()
