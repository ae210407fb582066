"""Timings of the blend-weighted-error pass (ViewShardedFitter.error_state, gr_error_view / gr_error_views) on one GPU,
and the golden fit under the three densification rules.

1. One error_state() over all views through the native executor and through the Python schedule, in alternating windows
   after a warm-up (a host clock around work that ends in a device synchronise; the median window and [min .. max]),
   beside one contribution_state() and one L1 fit step of the same fitter; the cost as a share of a fit at a given
   densify interval.
2. --kernel-loop: only a loop of forward_native + contrib_view_native + error_view_native calls on one view, for a
   kernel trace in a run of its own (rocprofv3 --kernel-trace --stats -- python tools/error_bench.py --kernel-loop;
   tools/kstats.py): k_error_view and k_error_gather beside the same view's forward splat and k_contrib_view.
3. --golden: fit_multiview.main on tests/golden/fit_targets (300 steps, defaults) with --densify_mode opacity, gradient
   and error: final loss, final N, and the err percentiles at each densify (recorded, not asserted).

    python tools/error_bench.py [--gaussians 1000000 --views 50 --res 800] [--reps 3] [--windows 5] [--label C4]
                                [--interval 80] [--out FILE (appended)] [--kernel-loop | --golden]
"""
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


def kernel_loop(n, R, calls, dev):
    p = bench.synthetic_params(n, dev)
    m, s, c, o = (t.detach().contiguous() for t in fm.activations(p))
    cam = fm.orbit_cameras(3, R, R, dev)[1]
    gv = tr.make_view(cam.view, cam.proj, R, R, None, depth_grad=False)
    target = torch.rand((R, R, 3), generator=torch.Generator(device=dev).manual_seed(3), device=dev)
    peak, err = torch.zeros((n,), device=dev), torch.zeros((n,), device=dev)
    for _ in range(calls):
        pv = tr.prepare_native(m, s, c, o, gv)
        _, _, _, rs = tr.forward_native(m, s, c, o, gv, pv, images=False)
        tr.contrib_view_native(rs, pv, peak)
        tr.error_view_native(rs, pv, target, err)
    torch.cuda.synchronize()
    print(f"kernel loop: {calls} x (prepare, gr_fwd_render, gr_contrib_view, gr_error_view) at {R}x{R}, {n} Gaussians, "
          f"{rs.plan.num_pairs} pairs ({rs.plan.num_core_pairs} core); {int((err > 0).sum())} Gaussians with error")


def golden(out):
    """The golden three-view fit under the three densification rules, through the CLI's main()."""
    lines = ["golden three-view fit (tests/golden/fit_targets), 300 steps, CLI defaults (128x128, 800 Gaussians, cap 3000), "
             f"on {'the HIP device' if torch.cuda.is_available() else 'host tensors'}; one run per mode, recorded and not "
             "asserted"]
    base = fm.ViewShardedFitter
    for mode in ("opacity", "gradient", "error"):
        log = []

        class Spy(base):
            def densify_and_prune(self, *a, **kw):
                n0 = int(self.params["means"].shape[0])
                super().densify_and_prune(*a, **kw)
                log.append((n0, dict(self.error_report) if kw.get("mode") == "error" else None, int(self.params["means"].shape[0])))

        fm.ViewShardedFitter = Spy
        try:
            with tempfile.TemporaryDirectory() as d:
                fm.main(["--targets_dir", os.path.join(REPO, "tests", "golden", "fit_targets"), "--out_dir", d, "--iters", "300",
                         "--seed", "1", "--densify_mode", mode])
                loss = [float(x) for x in open(os.path.join(d, "loss.txt")).read().split()]
        finally:
            fm.ViewShardedFitter = base
        lines.append(f"  --densify_mode {mode}: final loss {loss[-1]:.5f}, final N {log[-1][2]}")
        for k, (n0, r, n1) in enumerate(log):
            if r is None:
                lines.append(f"    densify {k + 1} (iter {80 * (k + 1)}): N {n0} -> {n1}")
            else:
                lines.append(f"    densify {k + 1} (iter {80 * (k + 1)}): N {n0}, err p50 {r['p50']:.3e} p90 {r['p90']:.3e} p99 "
                             f"{r['p99']:.3e} max {r['max']:.3e}; {r['clones']} cloned, {r['splits']} split; N -> {n1}")
    text = "\n".join(lines) + "\n"
    print(text)
    if out:
        with open(out, "a") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--views", type=int, default=50)
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--reps", type=int, default=3, help="calls (or fit steps x 5) per window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--interval", type=int, default=80, help="the densify interval the share of a fit is stated for")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--kernel-loop", action="store_true")
    ap.add_argument("--golden", action="store_true")
    args = ap.parse_args()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.golden:
        return golden(args.out)
    if not torch.cuda.is_available():
        raise SystemExit("error_bench: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda", 0)
    R = args.res
    if args.kernel_loop:
        return kernel_loop(args.gaussians, R, 20, dev)
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
            return fit.error_state()
        finally:
            fm.NATIVE_EXEC = saved

    ways = {"executor (gr_error_views)": lambda: state("1"), "Python schedule": lambda: state("0"),
            "contribution_state()": fit.contribution_state}
    res = {k: f() for k, f in ways.items()}  # warm-up, and the agreement of the two schedules
    a, b = res["executor (gr_error_views)"], res["Python schedule"]
    same = torch.equal(a, b)
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
    key = "executor (gr_error_views)" if fit._native_exec() else "Python schedule"
    q = torch.quantile(a.float().cpu(), torch.tensor([0.5, 0.9, 0.99])).tolist()
    lines.append(f"  one L1 fit step               : {ms:9.3f} ms  [{min(step):.3f} .. {max(step):.3f}]  (windows of {5 * args.reps} "
                 f"steps); error_state() as the fitter's defaults run it ({key}) = {med[key] / ms:.2f} fit steps = "
                 f"{med[key] / med['contribution_state()']:.2f} contribution_state() = {100.0 * med[key] / (args.interval * ms):.2f} % "
                 f"of a fit that densifies every {args.interval} steps")
    lines.append(f"  executor and Python schedule {'bit-identical' if same else 'DIFFER'}; err p50 {q[0]:.3e} p90 {q[1]:.3e} p99 "
                 f"{q[2]:.3e} max {float(a.max()):.3e}, {int((a == 0).sum())} of {a.numel()} without error (never seen)")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
