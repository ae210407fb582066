"""What tools/contribution_bench.py and tools/error_bench.py share: the arguments, the fitter, the alternating-window
timer of a per-Gaussian state call through the native executor and through the Python schedule, the one-view kernel
loop and the recorder of golden fits through the CLI's main()."""
import argparse
import importlib
import os
import statistics
import sys
import tempfile
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
fm = importlib.import_module("3dgaussian_amd.fit_multiview")
tr = importlib.import_module("3dgaussian_amd.torch_renderer")
bench = importlib.import_module("bench")


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def emit(lines, out):
    text = "\n".join(lines) + "\n"
    print(text)
    if out:
        with open(out, "a") as f:
            f.write(text)


def kernel_loop(n, R, calls, dev, error):
    """prepare, gr_fwd_render and gr_contrib_view (error: and gr_error_view) on one view, ``calls`` times."""
    p = bench.synthetic_params(n, dev)
    m, s, c, o = (t.detach().contiguous() for t in fm.activations(p))
    cam = fm.orbit_cameras(3, R, R, dev)[1]
    gv = tr.make_view(cam.view, cam.proj, R, R, None, depth_grad=False)
    target = torch.rand((R, R, 3), generator=torch.Generator(device=dev).manual_seed(3), device=dev) if error else None
    peak, err = torch.zeros((n,), device=dev), torch.zeros((n,), device=dev)
    for _ in range(calls):
        pv = tr.prepare_native(m, s, c, o, gv)
        _, _, _, rs = tr.forward_native(m, s, c, o, gv, pv, images=False)
        tr.contrib_view_native(rs, pv, peak)
        if error:
            tr.error_view_native(rs, pv, target, err)
    torch.cuda.synchronize()
    seen = f"{int((err > 0).sum())} Gaussians with error" if error else f"{int((peak > 0).sum())} Gaussians with a pair"
    print(f"kernel loop: {calls} x (prepare, gr_fwd_render, gr_contrib_view{', gr_error_view' if error else ''}) at {R}x{R}, "
          f"{n} Gaussians, {rs.plan.num_pairs} pairs ({rs.plan.num_core_pairs} core); {seen}")


def golden(out, header, runs, spy, describe):
    """The golden three-view fit (300 steps, seed 1) through the CLI's main(), once per entry of ``runs`` (mode -> its
    extra CLI arguments).  ``spy(fitter, a, kw, run)`` wraps every densify_and_prune (``run()`` makes the call) and
    returns that call's log entry; ``describe(mode, loss, log)`` gives the mode's lines."""
    lines = [header]
    base = fm.ViewShardedFitter
    for mode, extra in runs.items():
        log = []

        class Spy(base):
            def densify_and_prune(self, *a, **kw):
                log.append(spy(self, a, kw, lambda: super(Spy, self).densify_and_prune(*a, **kw)))

        fm.ViewShardedFitter = Spy
        try:
            with tempfile.TemporaryDirectory() as d:
                fm.main(["--targets_dir", os.path.join(REPO, "tests", "golden", "fit_targets"), "--out_dir", d, "--iters", "300",
                         "--seed", "1"] + extra)
                loss = [float(x) for x in open(os.path.join(d, "loss.txt")).read().split()]
        finally:
            fm.ViewShardedFitter = base
        lines += describe(mode, loss, log)
    emit(lines, out)


def parse_args(extra=lambda ap: None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--views", type=int, default=50)
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--reps", type=int, default=3, help="calls (or fit steps x 5) per window")
    ap.add_argument("--windows", type=int, default=5)
    extra(ap)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--kernel-loop", action="store_true")
    ap.add_argument("--golden", action="store_true")
    args = ap.parse_args()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    return args


def measure(args, dev, method, executor, beside):
    """The fitter of the arguments after three steps; ``method`` (a fitter method's name) through the executor
    (``executor``: that way's label) and through the Python schedule beside the fitter method ``beside``, in alternating
    windows, and the fit step.  Returns the report's first lines, the medians by way, the step's median, the label of the
    way the fitter's defaults take, the executor's result and whether the Python schedule's equals it."""
    R = args.res
    cams = fm.orbit_cameras(args.views, R, R, dev)
    g = torch.Generator(device=dev).manual_seed(3)
    targets = [torch.rand((R, R, 3), generator=g, device=dev) for _ in cams]
    masks = [(t.mean(dim=2) > 0.5).float() for t in targets]
    fit = fm.ViewShardedFitter(bench.synthetic_params(args.gaussians, dev), cams, targets, R, R, masks=masks)
    for _ in range(3):
        fit.step()
    fit.graph_sync()

    def state(native):
        saved = fm.NATIVE_EXEC
        fm.NATIVE_EXEC = native
        try:
            return getattr(fit, method)()
        finally:
            fm.NATIVE_EXEC = saved

    ways = {executor: lambda: state("1"), "Python schedule": lambda: state("0"), beside + "()": getattr(fit, beside)}
    res = {k: f() for k, f in ways.items()}  # warm-up, and the agreement of the two schedules
    a = res[executor]
    same = torch.equal(a, res["Python schedule"])
    times = {k: [] for k in ways}
    for _ in range(args.windows):
        for k, f in ways.items():
            times[k].append(timed(f, args.reps))
    step = [timed(fit.step, 5 * args.reps) for _ in range(args.windows)]
    fit.graph_sync()
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = [f"{args.label + ': ' if args.label else ''}{args.gaussians} Gaussians, {args.views} views, {R}x{R}, "
             f"{torch.cuda.get_device_name(0)}; {args.windows} alternating windows of {args.reps} calls after one warm-up each, "
             "median ms per call over all views [min .. max]"]
    for k in ways:
        lines.append(f"  {k:28s}: {med[k]:9.3f} ms  [{min(times[k]):.3f} .. {max(times[k]):.3f}]  {med[k] / args.views:.3f} ms per view")
    ms = statistics.median(step)
    key = executor if fit._native_exec() else "Python schedule"
    lines.append(f"  one L1 fit step               : {ms:9.3f} ms  [{min(step):.3f} .. {max(step):.3f}]  (windows of {5 * args.reps} "
                 f"steps); {method}() as the fitter's defaults run it ({key}) = {med[key] / ms:.2f} fit steps = "
                 f"{med[key] / med[beside + '()']:.2f} {beside}()")
    return lines, med, ms, key, a, same
