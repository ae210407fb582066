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
import torch

from state_bench_common import emit, golden, kernel_loop, measure, parse_args


def golden_spy(fit, a, kw, run):
    n0 = int(fit.params["means"].shape[0])
    run()
    return n0, dict(fit.error_report) if kw.get("mode") == "error" else None, int(fit.params["means"].shape[0])


def golden_lines(mode, loss, log):
    lines = [f"  --densify_mode {mode}: final loss {loss[-1]:.5f}, final N {log[-1][2]}"]
    for k, (n0, r, n1) in enumerate(log):
        if r is None:
            lines.append(f"    densify {k + 1} (iter {80 * (k + 1)}): N {n0} -> {n1}")
        else:
            lines.append(f"    densify {k + 1} (iter {80 * (k + 1)}): N {n0}, err p50 {r['p50']:.3e} p90 {r['p90']:.3e} p99 "
                         f"{r['p99']:.3e} max {r['max']:.3e}; {r['clones']} cloned, {r['splits']} split; N -> {n1}")
    return lines


def main():
    args = parse_args(lambda ap: ap.add_argument("--interval", type=int, default=80,
                                                 help="the densify interval the share of a fit is stated for"))
    if args.golden:
        return golden(args.out, "golden three-view fit (tests/golden/fit_targets), 300 steps, CLI defaults (128x128, 800 "
                      f"Gaussians, cap 3000), on {'the HIP device' if torch.cuda.is_available() else 'host tensors'}; one run "
                      "per mode, recorded and not asserted",
                      {mode: ["--densify_mode", mode] for mode in ("opacity", "gradient", "error")}, golden_spy, golden_lines)
    if not torch.cuda.is_available():
        raise SystemExit("error_bench: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda", 0)
    if args.kernel_loop:
        return kernel_loop(args.gaussians, args.res, 20, dev, error=True)
    lines, med, ms, key, a, same = measure(args, dev, "error_state", "executor (gr_error_views)", "contribution_state")
    lines[-1] += f" = {100.0 * med[key] / (args.interval * ms):.2f} % of a fit that densifies every {args.interval} steps"
    q = torch.quantile(a.float().cpu(), torch.tensor([0.5, 0.9, 0.99])).tolist()
    lines.append(f"  executor and Python schedule {'bit-identical' if same else 'DIFFER'}; err p50 {q[0]:.3e} p90 {q[1]:.3e} p99 "
                 f"{q[2]:.3e} max {float(a.max()):.3e}, {int((a == 0).sum())} of {a.numel()} without error (never seen)")
    emit(lines, args.out)


if __name__ == "__main__":
    main()
