"""Timings of held-out evaluation (ViewShardedFitter.evaluate, gr_eval_view / gr_eval_views) on one GPU.

1. One evaluate() over all views, three ways, in alternating windows after a warm-up (a host clock around work that
   ends in a device synchronise; the median window and [min .. max]): the native executor (gr_eval_views), the Python
   schedule of the same calls, and the composed route (render_gaussians_torch + losses.image_metrics per view);
   beside them one fit step of the same fitter (the L1 fit), so that a user can choose --eval_interval.
2. gr_eval_view alone (k_eval_view + k_eval_final) on one view's saved sums, `--calls` calls back to back between two
   device events, the saved sums and targets rotated over `--sets` buffers (a call does not find its inputs in the
   Infinity Cache); set beside a byte model: 16 B of saved sums + 12 B of target per pixel, the 5-pixel halo's
   re-reads counted ((26 / 16)^2 of the pixels at interior tiles), as a fraction of the HBM peak.
3. --kernel-loop: only a loop of gr_eval_view and gr_bwd_fit_ssim_gather calls on one view, for a kernel trace
   (rocprofv3 --kernel-trace --stats -- python tools/eval_bench.py --kernel-loop; tools/kstats.py): k_eval_view
   beside k_ssim_fwd_saved, in alternating order.
4. --color_correct: instead of 1 and 2, evaluate(color_correct=True) against evaluate() of the same fitter, through the
   executor (gr_eval_views_cc / gr_eval_views) and the Python schedule, in alternating windows; with --kernel-loop a
   loop of the three per-view calls (gr_eval_view, gr_cc_fit_view, gr_eval_view_cc) for a kernel trace.
5. --masked: the same for evaluate(masks=True) (gr_eval_views_masked / gr_eval_views); with --kernel-loop a loop of the two
   per-view calls (gr_eval_view, gr_eval_view_masked): k_eval_view_masked beside k_eval_view.

    python tools/eval_bench.py [--gaussians 1000000 --views 50 --res 800] [--reps 3] [--windows 5] [--label C4]
                               [--out FILE (appended)] [--kernel-loop] [--color_correct | --masked]
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
losses = importlib.import_module("3dgaussian_amd.losses")
bench = importlib.import_module("bench")

HBM_SPEC, HBM_ACHIEVABLE = 8.0e12, 6.3e12  # bytes / s


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def composed(fit, cams, targets):
    """The composed route: the drop-in op's image, then image_metrics, per view; the host reads the results once."""
    dev = targets[0].device
    with torch.no_grad():
        p = fit.canonical_params()
        m, s, c, o = (t.detach() for t in fm.activations(p))
        rows = []
        for cam, t in zip(cams, targets):
            img = tr.render_gaussians_torch(m, s, c, o, cam, width=fit.width, height=fit.height, background=fit._background(dev),
                                            max_gaussians=max(10000, int(m.shape[0])), depth_grad=False)
            mt = losses.image_metrics(img, t)
            rows.append(torch.stack([mt["l1"], mt["mse"], mt["ssim"]]))
        return torch.stack(rows).double().cpu().numpy()


def view_state(n, R, dev):
    p = bench.synthetic_params(n, dev)
    m, s, c, o = (t.detach().contiguous() for t in fm.activations(p))
    cam = fm.orbit_cameras(3, R, R, dev)[1]
    gv = tr.make_view(cam.view, cam.proj, R, R, None, depth_grad=False)
    _, _, _, st = tr.forward_native(m, s, c, o, gv, images=False)
    return (m, s, c, o), st


def kernel_lines(n, R, calls, sets, dev):
    _, st = view_state(n, R, dev)
    g = torch.Generator(device=dev).manual_seed(1)
    saved = [st.saved.clone() for _ in range(sets)]
    targets = [torch.rand((R, R, 3), generator=g, device=dev) for _ in range(sets)]
    out = torch.zeros(3, device=dev)
    states = [tr.RenderState(st.gv, st.n, st.plan, st.geom, st.bins, sv) for sv in saved]
    run = lambda q: tr.eval_view_native(states[q % sets], targets[q % sets], out)  # noqa: E731
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
        times.append(1e3 * e0.elapsed_time(e1) / calls)  # us per call
    us = statistics.median(times)
    tiles = ((R + 15) // 16) ** 2
    once, halo = 28 * R * R, 28 * min(26 * 26 * tiles, R * R * (26 / 16) ** 2)
    return [f"gr_eval_view alone (k_eval_view + k_eval_final), {R}x{R}, {calls} calls back to back over {sets} buffer sets, "
            f"device events: {us:.1f} us per call [{min(times):.1f} .. {max(times):.1f}]",
            f"  byte model: {once / 1e6:.1f} MB read once (16 B saved sums + 12 B target per pixel) = {once / us / 1e6:.2f} TB/s "
            f"({100 * once / us / 1e6 / (HBM_SPEC / 1e12):.0f}% of the 8 TB/s spec); with the halo re-reads {halo / 1e6:.1f} MB = "
            f"{halo / us / 1e6:.2f} TB/s requested (the re-reads are served by the caches)"]


# --kernel-loop: the per-view calls of a variant, each f(st, target, mask, row) on one view's state, and their label.
# plain: gr_eval_view beside the fused D-SSIM backward, alternated; the others: the calls of gr_eval_views_cc /
# gr_eval_views_masked in order (row: the view's row of that pass, the transform at 6).
KERNEL_LOOPS = {
    "plain": ([lambda st, t, m, row: tr.eval_view_native(st, t, row[:3]),
               lambda st, t, m, row: tr.backward_fit_ssim_gather_native(st, t, None, 0.0, None, 0.0, 1.0, 0.2, row[3:4])],
              "gr_eval_view, gr_bwd_fit_ssim_gather", True),
    "cc": ([lambda st, t, m, row: tr.eval_view_native(st, t, row[:3]),
            lambda st, t, m, row: tr.cc_fit_view_native(st, t, row[6:]),
            lambda st, t, m, row: tr.eval_view_cc_native(st, t, row[6:], row[3:6])],
           "gr_eval_view, gr_cc_fit_view, gr_eval_view_cc", False),
    "masked": ([lambda st, t, m, row: tr.eval_view_native(st, t, row[:3]),
                lambda st, t, m, row: tr.eval_view_masked_native(st, t, m, row[3:9])],
               "gr_eval_view, gr_eval_view_masked", False),
}


def kernel_loop(n, R, calls, dev, per_view, label, alternate):
    """--kernel-loop: `calls` rounds of one view's per-view calls, for a kernel trace.  alternate: every other round in
    reverse (E B B E E B ...: each kernel as often behind the other, its inputs in cache, as behind a backward)."""
    _, st = view_state(n, R, dev)
    target = torch.rand((R, R, 3), device=dev)
    mask = (target.mean(dim=2) > 0.5).float()
    row = torch.zeros(18, device=dev)
    for i in range(calls):
        for f in (per_view[::-1] if alternate and i % 2 else per_view):
            f(st, target, mask, row)
    torch.cuda.synchronize()
    print(f"kernel loop: {calls} x ({label}) at {R}x{R}, {n} Gaussians")


def option_lines(fit, args, R, name, kw, tail):
    """--color_correct, --masked: evaluate(**kw) (``name`` in the lines) against evaluate() of the same fitter, the
    executor and the Python schedule, in alternating windows; ``tail(result)``: the end of the last line."""
    def evaluate(native, on):
        saved = fm.NATIVE_EXEC
        fm.NATIVE_EXEC = native
        try:
            return fit.evaluate(**(kw if on else {}))
        finally:
            fm.NATIVE_EXEC = saved

    ways = {"executor, plain": lambda: evaluate("1", False), f"executor, {name}": lambda: evaluate("1", True),
            "Python schedule, plain": lambda: evaluate("0", False), f"Python schedule, {name}": lambda: evaluate("0", True)}
    res = {k: f() for k, f in ways.items()}  # warm-up, and the agreement
    a, b = res[f"executor, {name}"], res[f"Python schedule, {name}"]
    same = all((a[k] == b[k]).all() for k in a if hasattr(a[k], "all"))
    plain_same = all((a[k] == res["executor, plain"][k]).all() for k in ("l1", "mse", "ssim"))
    times = {k: [] for k in ways}
    for _ in range(args.windows):
        for k, f in ways.items():
            times[k].append(timed(f, args.reps))
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = [f"{args.label + ': ' if args.label else ''}{args.gaussians} Gaussians, {args.views} views, {R}x{R}, "
             f"{torch.cuda.get_device_name(0)}; {args.windows} alternating windows of {args.reps} evaluations after one warm-up "
             "each, median ms per evaluate() over all views [min .. max]"]
    for k in ways:
        lines.append(f"  {k:32s}: {med[k]:9.3f} ms  [{min(times[k]):.3f} .. {max(times[k]):.3f}]  "
                     f"{1e3 * med[k] / args.views:.1f} us per view")
    for w in ("executor", "Python schedule"):
        d = med[f"{w}, {name}"] - med[w + ", plain"]
        lines.append(f"  {w}: {name} adds {1e3 * d / args.views:.1f} us per view "
                     f"({med[f'{w}, {name}'] / med[w + ', plain']:.3f}x)")
    lines.append(f"  executor and Python schedule {'bit-identical' if same else 'DIFFER'}; plain keys "
                 f"{'unchanged by the argument' if plain_same else 'DIFFER'}; mean PSNR {a['mean_psnr']:.3f} dB, {tail(a)}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--views", type=int, default=50)
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--reps", type=int, default=3, help="evaluations (or fit steps x 5) per window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--sets", type=int, default=24)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--kernel-loop", action="store_true")
    ap.add_argument("--no-kernel", action="store_true", help="skip part 2")
    ap.add_argument("--color_correct", action="store_true",
                    help="instead of parts 1 and 2: evaluate(color_correct=True) against evaluate() (executor and Python "
                         "schedule); with --kernel-loop: the three per-view calls of gr_eval_views_cc")
    ap.add_argument("--masked", action="store_true",
                    help="instead of parts 1 and 2: evaluate(masks=True) against evaluate() (executor and Python schedule); "
                         "with --kernel-loop: the two per-view calls of gr_eval_views_masked")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda", 0)
    R = args.res
    if args.kernel_loop:
        return kernel_loop(args.gaussians, R, 20, dev, *KERNEL_LOOPS["cc" if args.color_correct else "masked" if args.masked else "plain"])
    cams = fm.orbit_cameras(args.views, R, R, dev)
    g = torch.Generator(device=dev).manual_seed(3)
    targets = [torch.rand((R, R, 3), generator=g, device=dev) for _ in cams]
    masks = [(t.mean(dim=2) > 0.5).float() for t in targets]
    fit = fm.ViewShardedFitter(bench.synthetic_params(args.gaussians, dev), cams, targets, R, R, masks=masks)
    for _ in range(3):
        fit.step()
    fit.graph_sync()
    if args.color_correct or args.masked:
        if args.color_correct:
            lines = option_lines(fit, args, R, "color_correct", dict(color_correct=True),
                                 lambda a: f"corrected {a['mean_cc_psnr']:.3f} dB")
        else:
            lines = option_lines(fit, args, R, "masked", dict(masks=True),
                                 lambda a: f"masked {a['mean_fg_psnr']:.3f} dB, silhouette IoU {a['mean_sil_iou']:.4f}")
        text = "\n".join(lines) + "\n"
        print(text)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(text)
        return

    def evaluate(native):
        saved = fm.NATIVE_EXEC
        fm.NATIVE_EXEC = native
        try:
            return fit.evaluate()
        finally:
            fm.NATIVE_EXEC = saved

    ways = {"executor (gr_eval_views)": lambda: evaluate("1"), "Python schedule": lambda: evaluate("0"),
            "composed route": lambda: composed(fit, cams, targets)}
    res = {k: f() for k, f in ways.items()}  # warm-up, and the agreement of the three
    a, b, cmp = res["executor (gr_eval_views)"], res["Python schedule"], res["composed route"]
    same = all((a[k] == b[k]).all() for k in ("l1", "mse", "ssim"))
    diff = [float(abs(a[k] - cmp[:, i]).max()) for i, k in enumerate(("l1", "mse", "ssim"))]
    times = {k: [] for k in ways}
    for _ in range(args.windows):
        for k, f in ways.items():
            times[k].append(timed(f, args.reps))
    # the fit step in windows of its own afterwards: an evaluation changes nothing of the fit
    step = [timed(fit.step, 5 * args.reps) for _ in range(args.windows)]
    fit.graph_sync()
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = [f"{args.label + ': ' if args.label else ''}{args.gaussians} Gaussians, {args.views} views, {R}x{R}, "
             f"{torch.cuda.get_device_name(0)}; {args.windows} alternating windows of {args.reps} evaluations after one warm-up "
             "each, median ms per evaluate() over all views [min .. max]"]
    for k in ways:
        lines.append(f"  {k:26s}: {med[k]:9.3f} ms  [{min(times[k]):.3f} .. {max(times[k]):.3f}]  "
                     f"{med[k] / args.views:.3f} ms per view")
    ms = statistics.median(step)
    key = "executor (gr_eval_views)" if fit._native_exec() else "Python schedule"
    lines.append(f"  one L1 fit step              : {ms:9.3f} ms  [{min(step):.3f} .. {max(step):.3f}]  "
                 f"(windows of {5 * args.reps} steps); evaluate() as the fitter's defaults run it ({key}) = "
                 f"{med[key] / ms:.2f} fit steps")
    lines.append(f"  composed / executor {med['composed route'] / med['executor (gr_eval_views)']:.2f}x, composed / Python schedule "
                 f"{med['composed route'] / med['Python schedule']:.2f}x; executor and Python schedule "
                 f"{'bit-identical' if same else 'DIFFER'}; max |kernel - composed| l1 {diff[0]:.2e} mse {diff[1]:.2e} "
                 f"ssim {diff[2]:.2e}; mean PSNR {a['mean_psnr']:.3f} dB, SSIM {a['mean_ssim']:.5f}")
    if not args.no_kernel:
        lines += kernel_lines(args.gaussians, R, args.calls, args.sets, dev)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
