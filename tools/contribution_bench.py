"""Timings of the peak-blend-weight pass (ViewShardedFitter.contribution_state, gr_contrib_view / gr_contrib_views) on one
GPU, and the golden fit under the two pruning rules.

1. One contribution_state() over all views through the native executor and through the Python schedule, in alternating
   windows after a warm-up (a host clock around work that ends in a device synchronise; the median window and
   [min .. max]), beside one evaluate() and one fit step of the same fitter.
2. --kernel-loop: only a loop of forward_native + contrib_view_native calls on one view, for a kernel trace in a run of
   its own (rocprofv3 --kernel-trace --stats -- python tools/contribution_bench.py --kernel-loop; tools/kstats.py):
   k_contrib_view and k_contrib_gather beside the same view's forward splat.
3. --golden: fit_multiview.main on tests/golden/fit_targets (300 steps, gradient densify) with --prune_mode opacity and
   contribution: final loss, final N, and per prune interval the Gaussians each rule removed (recorded, not asserted).

    python tools/contribution_bench.py [--gaussians 1000000 --views 50 --res 800] [--reps 3] [--windows 5] [--label C4]
                                       [--out FILE (appended)] [--kernel-loop | --golden]
"""
import torch

from state_bench_common import emit, golden, kernel_loop, measure, parse_args


def golden_spy(fit, a, kw, run):
    n0 = int(fit.params["means"].shape[0])
    by_op = int((torch.sigmoid(fit.params["opacities_raw"].detach()) <= a[2]).sum())
    run()
    r = getattr(fit, "contribution_report", None) if kw.get("prune_mode") == "contribution" else None
    return n0, by_op, r, int(fit.params["means"].shape[0])


def golden_lines(mode, loss, log):
    lines = [f"  --prune_mode {mode}: final loss {loss[-1]:.5f}, final N {log[-1][3]}"]
    for k, (n0, by_op, r, n1) in enumerate(log):
        if r is None:
            lines.append(f"    interval {k + 1} (iter {80 * (k + 1)}): N {n0}, the opacity rule pruned {by_op}; N -> {n1}")
        else:
            lines.append(f"    interval {k + 1} (iter {80 * (k + 1)}): N {n0}, the contribution rule pruned {r['pruned']} (peak "
                         f"p1 {r['p1']:.2e} p10 {r['p10']:.2e} p50 {r['p50']:.2e}); the opacity rule would have pruned "
                         f"{r['opacity_would_prune']} ({r['both']} in common); N -> {n1}")
    return lines


def main():
    args = parse_args()
    if args.golden:
        return golden(args.out, "golden three-view fit (tests/golden/fit_targets), 300 steps, --densify_mode gradient, CLI "
                      "defaults otherwise (128x128, 800 Gaussians, cap 3000), on "
                      f"{'the HIP device' if torch.cuda.is_available() else 'host tensors'}; one run per mode, recorded and not "
                      "asserted",
                      {mode: ["--densify_mode", "gradient", "--prune_mode", mode] for mode in ("opacity", "contribution")},
                      golden_spy, golden_lines)
    if not torch.cuda.is_available():
        raise SystemExit("contribution_bench: no HIP device (timings are taken on the GPU only)")
    dev = torch.device("cuda", 0)
    if args.kernel_loop:
        return kernel_loop(args.gaussians, args.res, 20, dev, error=False)
    lines, _, _, _, a, same = measure(args, dev, "contribution_state", "executor (gr_contrib_views)", "evaluate")
    q = torch.quantile(a.float().cpu(), torch.tensor([0.01, 0.1, 0.5, 0.99])).tolist()
    lines.append(f"  executor and Python schedule {'bit-identical' if same else 'DIFFER'}; peak p1 {q[0]:.2e} p10 {q[1]:.2e} p50 "
                 f"{q[2]:.2e} p99 {q[3]:.2e}, {int((a <= 1.0 / 510.0).sum())} of {a.numel()} at or below 1/510, "
                 f"{int((a == 0).sum())} never seen")
    emit(lines, args.out)


if __name__ == "__main__":
    main()
