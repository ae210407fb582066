"""CPU: gradient-driven densification (fit_multiview.densify_by_gradient, ViewShardedFitter(density_stats=True)).

* the rule on hand-built statistics: clone / split partition, prune and its 64-keep fallback, the cap (largest
  average first, ties to the lower index), output order and noise consumption, unseen rows, child scales, determinism;
* the host-tensor fit: density_state() is the sum over steps and views of the float64 dense statistic
  (tests/density_reference.py) at relL2 <= 1e-5 (float32 against float64 of the same dense math), survives a
  respatialize() unchanged, and over two gloo ranks equals the single-process state;
* a short --densify_mode gradient run of the CLI on the golden targets.
"""
from __future__ import annotations

import importlib
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (REPO, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import density_reference as dref  # noqa: E402
from conftest import GOLDEN  # noqa: E402


def _fm():
    return importlib.import_module("3dgaussian_amd.fit_multiview")


def _inv_softplus(s):
    return torch.log(torch.expm1(s - 1e-3))


def _params(n, scales=None, opac=0.5, seed=0):
    """Raw parameters with chosen activated scales (n, 3) and opacities."""
    g = torch.Generator().manual_seed(seed)
    s = torch.full((n, 3), 0.05) if scales is None else scales
    o = torch.full((n,), float(opac)) if not torch.is_tensor(opac) else opac
    return {"means": torch.rand((n, 3), generator=g) - 0.5, "scales_raw": _inv_softplus(s),
            "opacities_raw": torch.logit(o), "colors_raw": torch.rand((n, 3), generator=g)}


def test_clone_split_partition_by_split_scale():
    fm = _fm()
    n = 100
    s = torch.full((n, 3), 0.02)
    s[10:20, 0] = 0.3   # large in x
    s[20:30, 1] = 0.3   # large in y
    s[30:40, 2] = 0.3   # large in z only: the renderer does not read it, no split
    p = _params(n, s)
    gsum, seen = torch.ones(n), torch.ones(n)
    gsum[50:] = 0.0  # below the threshold
    noise = torch.randn((2 * n, 3), generator=torch.Generator().manual_seed(1))
    out = fm.densify_by_gradient(p, gsum, seen, 0.5, 0.1, 10_000, 0.05, noise=noise)
    # 50 candidates: 20 split (parents leave, 40 children), 30 cloned
    assert out["means"].shape[0] == n - 20 + 30 + 40
    surv = torch.cat([torch.arange(0, 10), torch.arange(30, n)])
    assert torch.equal(out["means"][:80], p["means"][surv])
    clones = torch.cat([torch.arange(0, 10), torch.arange(30, 50)])
    for k in p:
        assert torch.equal(out[k][80:110], p[k][clones]), k
    # a row at exactly split_scale is cloned (smax <= split_scale)
    s2 = torch.full((70, 3), 0.1)
    p2 = _params(70, s2)
    sm = (torch.nn.functional.softplus(p2["scales_raw"]) + 1e-3)[:, :2].max(dim=1).values
    out2 = fm.densify_by_gradient(p2, torch.ones(70), torch.ones(70), 0.5, float(sm.max()), 10_000, 0.05, noise=noise)
    assert out2["means"].shape[0] == 140 and torch.equal(out2["means"][70:], p2["means"])


def test_prune_and_keep64_fallback():
    fm = _fm()
    n = 200
    o = torch.full((n,), 0.5)
    o[::2] = 0.01
    p = _params(n, opac=o)
    out = fm.densify_by_gradient(p, torch.zeros(n), torch.zeros(n), 1.0, 0.1, 10_000, 0.05)
    assert out["means"].shape[0] == 100 and torch.equal(out["means"], p["means"][1::2])
    # fewer than 64 above the bar: the 64 most opaque stay, as the existing rule
    o = torch.linspace(0.001, 0.04, n)
    o[7] = 0.5
    p = _params(n, opac=o)
    out = fm.densify_by_gradient(p, torch.zeros(n), torch.zeros(n), 1.0, 0.1, 10_000, 0.05)
    ref = fm.densify_and_prune_device(p, 10_000, 0.0, 0.05)
    assert out["means"].shape[0] == 64
    for k in p:
        assert torch.equal(out[k], ref[k]), k
    # pruned rows are no candidates, whatever their gradient
    o = torch.full((n,), 0.5)
    o[:100] = 0.01
    p = _params(n, opac=o)
    out = fm.densify_by_gradient(p, torch.ones(n), torch.ones(n), 0.5, 1.0, 10_000, 0.05)
    assert out["means"].shape[0] == 200 and torch.equal(out["means"][100:], p["means"][100:])


def test_cap_takes_largest_avg_with_index_tie_break():
    fm = _fm()
    n = 100
    p = _params(n)
    gsum = torch.zeros(n)
    gsum[[5, 17, 40, 41, 90]] = torch.tensor([3.0, 2.0, 2.0, 2.0, 9.0])
    seen = torch.ones(n)
    # room for 3 of the 5 candidates: 90 (9), 5 (3), then the tie at 2 goes to the lowest index, 17
    out = fm.densify_by_gradient(p, gsum, seen, 1.0, 1.0, n + 3, 0.05)
    assert out["means"].shape[0] == n + 3
    assert torch.equal(out["means"][n:], p["means"][[5, 17, 90]])  # clones in parent (index) order
    # the average decides, not the sum: 41 seen once beats 5 seen four times
    seen2 = seen.clone()
    seen2[5] = 4.0
    out = fm.densify_by_gradient(p, gsum, seen2, 1.0, 1.0, n + 3, 0.05)
    assert torch.equal(out["means"][n:], p["means"][[17, 40, 90]])
    # no room: prune only; a cap below the kept count adds nothing
    for cap in (n, n - 10):
        assert fm.densify_by_gradient(p, gsum, seen, 1.0, 1.0, cap, 0.05)["means"].shape[0] == n
    # splits count one row net each
    s = torch.full((n, 3), 0.5)
    out = fm.densify_by_gradient(_params(n, s), gsum, seen, 1.0, 0.1, n + 3, 0.05, noise=torch.zeros((6, 3)))
    assert out["means"].shape[0] == n + 3


def test_output_order_and_noise_consumption():
    fm = _fm()
    n = 80
    s = torch.full((n, 3), 0.02)
    s[[3, 50, 61], 0] = torch.tensor([0.4, 0.5, 0.6])
    p = _params(n, s)
    gsum = torch.zeros(n)
    gsum[[3, 20, 50, 61, 70]] = 1.0
    noise = torch.randn((10, 3), generator=torch.Generator().manual_seed(5))
    out = fm.densify_by_gradient(p, gsum, torch.ones(n), 0.5, 0.1, 10_000, 0.05, noise=noise)
    surv = [i for i in range(n) if i not in (3, 50, 61)]
    assert out["means"].shape[0] == len(surv) + 2 + 6
    for k in p:
        assert torch.equal(out[k][:len(surv)], p[k][surv]), k
        assert torch.equal(out[k][len(surv):len(surv) + 2], p[k][[20, 70]]), k
    sa = torch.nn.functional.softplus(p["scales_raw"]) + 1e-3
    kids = out["means"][len(surv) + 2:]
    for q, parent in enumerate((3, 50, 61)):
        for c in range(2):  # the k-th split uses noise[2k], noise[2k + 1], over all three columns
            torch.testing.assert_close(kids[2 * q + c], p["means"][parent] + sa[parent] * noise[2 * q + c], rtol=0, atol=1e-7)
        for k in ("opacities_raw", "colors_raw"):  # children keep the parent's colour and opacity
            assert torch.equal(out[k][len(surv) + 2 + 2 * q], p[k][parent]) and torch.equal(out[k][len(surv) + 3 + 2 * q], p[k][parent])
    # rows of noise beyond 2 x splits are not read
    out2 = fm.densify_by_gradient(p, gsum, torch.ones(n), 0.5, 0.1, 10_000, 0.05, noise=noise[:6])
    assert torch.equal(out2["means"], out["means"])


def test_unseen_rows_are_never_candidates():
    fm = _fm()
    n = 70
    p = _params(n)
    gsum = torch.full((n,), 5.0)
    seen = torch.zeros(n)
    seen[:10] = 2.0
    out = fm.densify_by_gradient(p, gsum, seen, 0.0, 1.0, 10_000, 0.05)  # threshold 0: every seen row qualifies
    assert out["means"].shape[0] == n + 10 and torch.equal(out["means"][n:], p["means"][:10])


def test_child_scales_are_parent_over_1p6():
    fm = _fm()
    n = 70
    s = torch.rand((n, 3), generator=torch.Generator().manual_seed(2)) * 2.0 + 0.2
    s[0] = torch.tensor([30.0, 40.0, 25.0])   # above softplus' linear threshold
    s[1] = torch.tensor([0.2, 0.0012, 0.0011])  # s / 1.6 at or under the 1e-3 offset: the floor keeps the log finite
    p = _params(n, s)
    p["scales_raw"][1] = torch.tensor([float(_inv_softplus(torch.tensor(0.2))), -9.0, -12.0])
    out = fm.densify_by_gradient(p, torch.ones(n), torch.ones(n), 0.5, 0.1, 10_000, 0.05, noise=torch.zeros((2 * n, 3)))
    assert out["means"].shape[0] == 2 * n
    sa = torch.nn.functional.softplus(p["scales_raw"]) + 1e-3
    child = torch.nn.functional.softplus(out["scales_raw"]) + 1e-3
    assert torch.isfinite(out["scales_raw"]).all()
    want = (sa / 1.6).repeat_interleave(2, dim=0)
    ok = want > 2e-3  # (under the activation's 1e-3 offset the floor holds the scale at ~1e-3)
    torch.testing.assert_close(child[ok], want[ok], rtol=2e-6, atol=0)
    assert (child[~ok] >= 1e-3).all() and (child[~ok] <= 1.1e-3).all()


def test_same_noise_gives_bit_identical_results():
    fm = _fm()
    n = 300
    g = torch.Generator().manual_seed(9)
    s = torch.rand((n, 3), generator=g) * 0.3 + 0.01
    p = _params(n, s, opac=torch.rand(n, generator=g) * 0.9 + 0.02)
    gsum, seen = torch.rand(n, generator=g), torch.randint(0, 4, (n,), generator=g).float()
    noise = torch.randn((2 * n, 3), generator=g)
    a = fm.densify_by_gradient(p, gsum, seen, 0.1, 0.15, 420, 0.05, noise=noise)
    b = fm.densify_by_gradient(p, gsum, seen, 0.1, 0.15, 420, 0.05, noise=noise)
    assert a["means"].shape[0] <= 420
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # a generator in the same state draws the same children
    c = fm.densify_by_gradient(p, gsum, seen, 0.1, 0.15, 420, 0.05, generator=torch.Generator().manual_seed(3))
    d = fm.densify_by_gradient(p, gsum, seen, 0.1, 0.15, 420, 0.05, generator=torch.Generator().manual_seed(3))
    for k in c:
        assert torch.equal(c[k], d[k]), k


# ---- the host-tensor fit ---------------------------------------------------------------------------------------------
W, H, N, V = 64, 48, 300, 3


def _scene(n_views=V, n=N):
    fm = _fm()
    torch.manual_seed(7)
    params = fm.build_params(n, torch.device("cpu"), use_sh=False)
    cams = fm.orbit_cameras(n_views, W, H, torch.device("cpu"))
    g = torch.Generator().manual_seed(3)
    targets = [torch.rand((H, W, 3), generator=g) for _ in range(n_views)]
    masks = [(t.mean(2) > 0.5).float() for t in targets]
    return fm, params, cams, targets, masks


def _reference_step(fm, fit, cams, targets, masks):
    """The statistic of one step at the fitter's current parameters (canonical order), float64: (sum over views,
    per-view list)."""
    tr = importlib.import_module("3dgaussian_amd.torch_renderer")
    with torch.no_grad():
        m, s, c, o = (t.detach() for t in fm.activations(fit.canonical_params()))
        per = []
        for cam, tgt, msk in zip(cams, targets, masks):
            out, alpha, _ = tr.render_gaussians_torch(m, s, c, o, cam, W, H, background=torch.zeros(3), return_aux=True)
            g_out, g_alpha = dref.l1_upstream(out, alpha, tgt, msk, fit.w_sil, H, W)  # the kink's signs: the fit's images
            per.append((g_out, g_alpha, cam))
    return [dref.view_statistic(m, s, c, o, cam.view, cam.proj, W, H, g_out, g_alpha)[0] for g_out, g_alpha, cam in per]


@pytest.fixture(scope="module")
def cpu_fit():
    """Three steps of the f1-size fit with statistics, and the float64 reference's sums (computed once, shared)."""
    fm, params, cams, targets, masks = _scene()
    fit = fm.ViewShardedFitter(params, cams, targets, W, H, masks=masks, density_stats=True)
    ref, lo = torch.zeros(N, dtype=torch.float64), torch.full((N,), float("inf"), dtype=torch.float64)
    steps = 3
    for _ in range(steps):
        for st in _reference_step(fm, fit, cams, targets, masks):
            ref += st
            lo = torch.minimum(lo, st)
        fit.step()
    return fm, fit, ref, lo, steps


def test_cpu_fit_state_matches_float64_reference(cpu_fit):
    fm, fit, ref, lo, steps = cpu_fit
    gsum, seen = fit.density_state()
    rel = float((gsum.double() - ref).norm() / ref.norm())
    print(f"cpu fit density_state vs float64 dense reference after {steps} steps: relL2 {rel:.3e}")
    assert gsum.shape == (N,) and seen.shape == (N,)
    assert rel <= 1e-5
    # every view sees a Gaussian whose float64 gradient is representable in float32; none more than steps x views
    assert float(seen.max()) <= steps * V
    assert torch.equal(seen[lo > 1e-30], torch.full_like(seen[lo > 1e-30], steps * V))
    assert float(ref.min()) >= 0.0 and float(gsum.min()) >= 0.0


def test_respatialize_keeps_the_state(cpu_fit):
    fm, fit, *_ = cpu_fit
    g0, s0 = fit.density_state()
    with torch.no_grad():  # move the Gaussians so that the Morton order really changes
        fit.params["means"].copy_(fit.params["means"].flip(0))
    perm0 = fit.perm.clone()
    c0 = {k: v.detach().clone() for k, v in fit.canonical_params().items()}
    fit.respatialize()
    assert not torch.equal(fit.perm, perm0)
    g1, s1 = fit.density_state()
    assert torch.equal(g0, g1) and torch.equal(s0, s1)
    for k, v in fit.canonical_params().items():
        assert torch.equal(v.detach(), c0[k]), k


def test_state_needs_the_flag():
    fm, params, cams, targets, masks = _scene(n=40)
    fit = fm.ViewShardedFitter(params, cams, targets, W, H, masks=masks)
    with pytest.raises(ValueError, match="density_stats"):
        fit.density_state()
    with pytest.raises(ValueError, match="density_stats"):
        fit.densify_and_prune(100, 0.1, 0.05, mode="gradient")


def test_fitter_gradient_mode_densify_resets_the_window():
    fm, params, cams, targets, masks = _scene(n=120)
    fit = fm.ViewShardedFitter(params, cams, targets, W, H, masks=masks, density_stats=True)
    for _ in range(2):
        fit.step()
    gsum, seen = fit.density_state()
    thr = float((gsum / seen.clamp_min(1)).median())
    fit.densify_and_prune(150, 0.15, 0.05, mode="gradient", grad_threshold=thr, split_scale=0.01)
    n1 = fit.params["means"].shape[0]
    assert 120 < n1 <= 150
    g, s = fit.density_state()
    assert g.shape == (n1,) and float(g.abs().sum()) == 0.0 and float(s.sum()) == 0.0
    assert torch.isfinite(fit.step())
    g, s = fit.density_state()
    assert float(s.max()) == V and float(g.sum()) > 0.0
    # densify_ratio 0 (a prune-only call of the CLI) adds nothing
    fit.densify_and_prune(150, 0.0, 0.05, mode="gradient", grad_threshold=0.0, split_scale=0.01)
    assert fit.params["means"].shape[0] <= n1


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    fm, params, cams, targets, masks = _scene(n_views=4, n=60)
    fit = fm.ViewShardedFitter(params, cams, targets, W, H, masks=masks, density_stats=True)
    for _ in range(2):
        fit.step()
    gsum, seen = fit.density_state()
    out_q.put((rank, gsum.numpy().copy(), seen.numpy().copy()))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_rank_gloo_state_matches_single_process():
    fm, params, cams, targets, masks = _scene(n_views=4, n=60)
    ref = fm.ViewShardedFitter(params, cams, targets, W, H, masks=masks, density_stats=True)
    for _ in range(2):
        ref.step()
    g_ref, s_ref = ref.density_state()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {r: (g, s) for r, g, s in (q.get(timeout=240) for _ in procs)}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in (0, 1):
        # the same views' statistics, summed over the ranks; the second step's parameters differ by the collective's
        # summation order of the gradient (float32), so by rounding
        torch.testing.assert_close(torch.from_numpy(res[r][0]), g_ref, rtol=1e-4, atol=1e-9)
        assert np.array_equal(res[r][1], s_ref.numpy())
    assert np.array_equal(res[0][0], res[1][0])


def test_cli_gradient_mode_on_golden_targets(tmp_path, capsys):
    fm = _fm()
    fm.main(["--targets_dir", os.path.join(GOLDEN, "fit_targets"), "--out_dir", str(tmp_path), "--iters", "7",
             "--width", "48", "--height", "48", "--num_gaussians", "200", "--max_gaussians", "230",
             "--densify_interval", "3", "--prune_interval", "3", "--seed", "1234", "--device", "cpu",
             "--densify_mode", "gradient", "--densify_grad_threshold", "1e-6"])
    losses = np.array([float(x) for x in (tmp_path / "loss.txt").read_text().split()])
    assert losses.shape == (7,) and np.isfinite(losses).all()
    npz = np.load(tmp_path / "gaussians_fitted.npz")
    n = npz["means"].shape[0]
    assert 200 < n <= 230, n
    assert (tmp_path / "preview_view0.png").exists()
    ns = [int(line.split("N=")[1]) for line in capsys.readouterr().out.splitlines() if "N=" in line]
    assert ns and max(ns) <= 230
