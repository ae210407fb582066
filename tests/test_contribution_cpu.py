"""CPU: contribution-based pruning without a device.  cpu_renderer.peak_contribution against the float64 dense reference
(tests/contribution_reference.py), the removal bound peak / (1 - peak) in float64, prune_by_contribution and the densify
rules' ``keep`` argument, a scene in which the opacity rule and the contribution rule disagree both ways, the collective
over two gloo ranks, the C entries' argument checks that come before any launch, and fit_multiview.main with
--prune_mode contribution."""
from __future__ import annotations

import ctypes
import importlib
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import contribution_reference as cr
from conftest import GOLDEN, REPO

HERE = os.path.dirname(os.path.abspath(__file__))
W = H = 32
N = 60
TINY = float(np.finfo(np.float32).tiny)  # below it a float32 weight underflows where the float64 one does not


@pytest.fixture(scope="module")
def fm(pkg):
    return importlib.import_module("3dgaussian_amd.fit_multiview")


@pytest.mark.parametrize("w,h,n,sigma", [(32, 24, 80, 0.05), (17, 13, 7, 0.05), (40, 30, 200, 0.3)],
                         ids=["32x24", "17x13", "40x30-big"])
def test_peak_contribution_matches_float64(pkg, fm, w, h, n, sigma):
    m, s, c, o = cr.scene(n, seed=3, sigma=sigma)
    worst = 0.0
    for cam in fm.orbit_cameras(3, w, h, "cpu"):
        got = pkg.cpu_renderer.peak_contribution(m, s, o, cam.view, cam.proj, w, h)
        ref, _ = cr.peak_ref(m, s, o, cam.view, cam.proj, w, h)
        assert got.dtype == torch.float32 and tuple(got.shape) == (n + cr.DEAD,)
        err = (got.double() - ref).abs()
        assert bool((err <= 1e-5 * ref + TINY).all()), float((err / ref.clamp_min(TINY)).max())
        seen = ref > TINY  # (a float64 weight below float32's range is 0 in float32: covered by TINY above)
        worst = max(worst, float((err[seen] / ref[seen]).max()))
        assert bool((got[-cr.DEAD:] == 0).all()) and float(ref[-cr.DEAD:].max()) < 1e-100
        assert float(got[:n].min()) > 0.0 and float(got.max()) < 1.0
    print(f"peak_contribution {w}x{h} n={n}: worst relative error against float64 {worst:.2e}")


def test_removal_bound_in_float64(fm):
    """Removing Gaussian i moves no pixel by more than peak_i / (1 - peak_i): every Gaussian of a 32 x 24 scene, in
    float64 (1e-15: the rounding of the two float64 renders being compared)."""
    w, h, n = 32, 24, 40
    m, s, c, o = cr.scene(n, seed=5, sigma=0.08)
    cam = fm.orbit_cameras(3, w, h, "cpu")[1]
    bg = torch.tensor([0.2, 0.5, 0.7])
    peak, _ = cr.peak_ref(m, s, o, cam.view, cam.proj, w, h)
    tight = 0.0
    for i in range(n + cr.DEAD):
        d = cr.removal_change(m, s, c, o, cam.view, cam.proj, w, h, i, bg)
        bound = float(peak[i] / (1.0 - peak[i]))
        assert d <= bound + 1e-15, (i, d, bound)
        if bound > 0:
            tight = max(tight, d / bound)
    print(f"removal bound: the largest change / bound over {n} Gaussians is {tight:.3f}")
    assert 0.05 < tight <= 1.0  # (a bound that some Gaussian comes near)


def test_prune_by_contribution(fm):
    peak = torch.tensor([0.5, 0.001, 0.002, 0.0, 0.3])
    assert fm.prune_by_contribution(peak, 0.0015, min_keep=2).tolist() == [True, False, True, False, True]
    assert fm.prune_by_contribution(peak, 0.002, min_keep=0).tolist() == [True, False, False, False, True]  # strictly above
    # the floor: the min_keep largest, ties to the lower index
    peak = torch.tensor([0.1, 0.2, 0.1, 0.1, 0.0])
    assert fm.prune_by_contribution(peak, 0.5, min_keep=3).tolist() == [True, True, True, False, False]
    assert fm.prune_by_contribution(peak, 0.5, min_keep=10).tolist() == [True] * 5
    big = torch.linspace(0.0, 0.01, 200)
    k = fm.prune_by_contribution(big, 1.0)
    assert int(k.sum()) == 64 and bool(k[-64:].all())  # the default floor of 64
    assert int(fm.prune_by_contribution(big, 1.0 / 510.0).sum()) == int((big > 1.0 / 510.0).sum())


def _params(fm, n=300, seed=2):
    torch.manual_seed(seed)
    p = fm.build_params(n, torch.device("cpu"), use_sh=False)
    with torch.no_grad():
        p["opacities_raw"].copy_(torch.randn(n) * 2.0 - 2.0)  # both sides of the opacity threshold
    return p


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_keep_none_is_the_existing_rule(fm):
    """keep=None: the three rules' existing code path (same random stream, torch.equal); keep given: exactly those rows
    survive, the opacity threshold and its floor are not consulted."""
    p = _params(fm)
    n = p["means"].shape[0]
    op = torch.sigmoid(p["opacities_raw"].detach())
    assert 64 < int((op > 0.05).sum()) < n
    noise = torch.randn((2 * n, 3), generator=torch.Generator().manual_seed(4))
    gsum, seen = torch.rand(n, generator=torch.Generator().manual_seed(6)), torch.ones(n)
    keep = torch.zeros(n, dtype=torch.bool)
    keep[::7] = True  # 43 rows: fewer than the floor of 64
    inf = float("inf")
    rules = ((fm.densify_and_prune, lambda grow: (p, 400, 0.15 if grow else 0.0, 0.05), {}),
             (fm.densify_and_prune_device, lambda grow: (p, 400, 0.15 if grow else 0.0, 0.05), {"noise": noise}),
             (fm.densify_by_gradient, lambda grow: (p, gsum, seen, 0.5 if grow else inf, 0.01, 400, 0.05), {"noise": noise}))
    for rule, args, kw in rules:
        torch.manual_seed(9)
        a = rule(*args(True), **kw)
        torch.manual_seed(9)
        b = rule(*args(True), keep=None, **kw)
        _same(a, b)
        assert a["means"].shape[0] > int((op > 0.05).sum())  # (it grew: the random draws were compared too)
        only = rule(*args(False), keep=keep, **kw)  # nothing added: the survivors are exactly the mask's rows
        assert only["means"].shape[0] == int(keep.sum())
        for name in p:
            assert torch.equal(only[name], p[name].detach()[keep]), name
        with pytest.raises(ValueError):
            rule(*args(True), keep=keep[:-1], **kw)


def _disagreement_scene(fm):
    """40 Gaussians of opacity ~1 stacked at the origin with one of opacity 0.06 among them, one of opacity 0.04 alone
    over the background, and 70 ordinary ones (so that neither rule reaches its floor of 64)."""
    dev = torch.device("cpu")
    n = 40 + 1 + 1 + 70
    g = torch.Generator().manual_seed(8)
    means = torch.zeros((n, 3))
    means[41] = torch.tensor([0.9, 0.6, 0.0])
    means[42:] = (torch.rand((70, 3), generator=g) - 0.5) * torch.tensor([1.0, 1.0, 0.2]) + torch.tensor([-0.5, -0.5, 0.0])
    op = torch.full((n,), 0.999)
    op[40], op[41] = 0.06, 0.04
    op[42:] = 0.5
    scales = torch.full((n, 3), 0.05)
    p = {"means": means, "scales_raw": torch.log(torch.expm1(scales - 1e-3)), "opacities_raw": torch.logit(op),
         "colors_raw": torch.zeros((n, 3))}
    p = {k: torch.nn.Parameter(v.clone()) for k, v in p.items()}
    cams = fm.orbit_cameras(3, W, H, dev)
    targets = [torch.zeros((H, W, 3)) for _ in cams]
    return p, cams, targets, n


def test_the_two_rules_disagree_both_ways(fm):
    rows = {}
    for mode in ("opacity", "contribution"):
        p, cams, targets, n = _disagreement_scene(fm)
        fit = fm.ViewShardedFitter(p, cams, targets, W, H, reorder=False)
        if mode == "contribution":
            peak = fit.contribution_state()
            assert float(peak[40]) < 1.0 / 510.0 and abs(float(peak[40]) - 0.06 / 41.0) < 2e-4  # ~ 0.06 / (1 + W), W ~ 40
            assert float(peak[41]) > 0.03  # alone over the background: 0.04 / 1.04
            want = fm.prune_by_contribution(peak, 1.0 / 510.0)
        else:
            want = torch.sigmoid(p["opacities_raw"].detach()) > 0.05
        assert int(want.sum()) >= 64
        before = {k: v.detach().clone() for k, v in fit.canonical_params().items()}
        fit.densify_and_prune(10_000, 0.0, 0.05, prune_mode=mode)
        after = fit.canonical_params()
        for k in before:
            assert torch.equal(after[k].detach(), before[k][want]), (mode, k)
        rows[mode] = want
        if mode == "contribution":
            r = fit.contribution_report
            assert r["n"] == n and r["pruned"] == int((~want).sum()) and r["at_or_below"] == r["pruned"]
            assert r["opacity_would_prune"] == 1 and r["both"] == 0 and r["p1"] <= r["p10"] <= r["p50"]
    assert bool(rows["opacity"][40]) and not bool(rows["contribution"][40])  # buried: kept by opacity, pruned by contribution
    assert not bool(rows["opacity"][41]) and bool(rows["contribution"][41])  # faint but alone: the other way round
    assert int((~rows["opacity"]).sum()) == 1


def _golden_targets(fm, count=3):
    d = os.path.join(GOLDEN, "fit_targets")
    paths = sorted(os.path.join(d, f) for f in os.listdir(d) if f.endswith(".png"))[:count]
    assert len(paths) == count
    return [torch.from_numpy(fm._load_image(p, W, H)) for p in paths]


def _fitter(fm, n=N, **kw):
    torch.manual_seed(5)
    dev = torch.device("cpu")
    params = fm.build_params(n, dev, use_sh=False)
    with torch.no_grad():
        params["scales_raw"].fill_(-1.0)
        params["colors_raw"].add_(1.0)
    targets = _golden_targets(fm)
    cams = fm.orbit_cameras(len(targets), W, H, dev)
    return fm.ViewShardedFitter(params, cams, targets, W, H, **kw), cams, targets


def test_contribution_state_on_host_tensors(pkg, fm):
    """Canonical order under the Morton permutation, the maximum over the views, other cameras on request, and a fit
    left exactly as it was."""
    fit, cams, _ = _fitter(fm, density_stats=True)
    other, _, _ = _fitter(fm, density_stats=True)
    la, lb = [fit.step()], [other.step()]
    assert fit.perm is not None
    g0 = {k: v.grad.clone() for k, v in fit.params.items()}
    rng = torch.get_rng_state()
    peak = fit.contribution_state()
    assert torch.equal(rng, torch.get_rng_state())
    for k, v in fit.params.items():
        assert torch.equal(v.grad, g0[k])
    assert peak.dtype == torch.float32 and tuple(peak.shape) == (N,)
    with torch.no_grad():
        # exact against the per-view function on the fitter's own (Morton) order, put back into canonical order (the
        # order of the Gaussians moves the last bits of the weight sum); the float64 reference on the canonical ones
        own = fm.activations(fit.params)
        per = []
        for c in cams:
            x = pkg.cpu_renderer.peak_contribution(own[0], own[1], own[3], c.view, c.proj, W, H)
            y = torch.empty_like(x)
            y[fit.perm] = x
            per.append(y)
        m, s, _, o = fm.activations(fit.canonical_params())
        ref = cr.peak_ref_views(m, s, o, [(c.view, c.proj) for c in cams], W, H)
    assert torch.equal(peak, torch.stack(per).max(dim=0).values)
    assert bool(((peak.double() - ref).abs() <= 1e-5 * ref + TINY).all())
    assert torch.equal(fit.contribution_state([cams[2]]), per[2])
    la += [fit.step() for _ in range(2)]
    lb += [other.step() for _ in range(2)]
    for x, y in zip(la, lb):
        assert torch.equal(x, y)
    for k in fit.params:
        assert torch.equal(fit.params[k], other.params[k]), k
    for x, y in zip(fit.density_state(), other.density_state()):
        assert torch.equal(x, y)


def test_opacity_mode_is_the_call_without_the_argument(fm):
    a, _, _ = _fitter(fm)
    b, _, _ = _fitter(fm)
    for f, kw in ((a, {}), (b, {"prune_mode": "opacity", "prune_contribution": 0.5})):
        f.step()
        torch.manual_seed(3)
        f.densify_and_prune(200, 0.15, 0.05, **kw)
        assert not hasattr(f, "contribution_report")
    _same({k: v.detach() for k, v in a.params.items()}, {k: v.detach() for k, v in b.params.items()})
    with pytest.raises(ValueError):
        a.densify_and_prune(200, 0.15, 0.05, prune_mode="peak")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


NR = 120  # Gaussians of the two-rank test: above the floor of 64, so that the threshold decides


def _worker(rank, world, port, thr, out_q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, REPO)
    sys.path.insert(0, HERE)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    fm = importlib.import_module("3dgaussian_amd.fit_multiview")
    fit, _, _ = _fitter(fm, NR)
    peak = fit.contribution_state()
    fit.densify_and_prune(200, 0.0, 0.05, prune_mode="contribution", prune_contribution=thr)
    out_q.put((rank, peak.numpy().copy(), fit.canonical_params()["means"].detach().numpy().copy(), fit.contribution_report))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_gloo_ranks_return_the_single_process_state(fm):
    fit, _, _ = _fitter(fm, NR)
    want = fit.contribution_state()
    thr = float(want.sort().values[30])  # the 31 smallest go
    fit.densify_and_prune(200, 0.0, 0.05, prune_mode="contribution", prune_contribution=thr)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, thr, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {r: rest for r, *rest in (q.get(timeout=240) for _ in procs)}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in (0, 1):
        assert np.array_equal(res[r][0], want.numpy())
        assert np.array_equal(res[r][1], fit.canonical_params()["means"].detach().numpy())
        assert res[r][2] == fit.contribution_report
    assert fit.contribution_report["pruned"] == 31 and fit.params["means"].shape[0] == NR - 31


def test_abi_argument_checks(pkg):
    """gr_contrib_ws_bytes and the checks of gr_contrib_view / gr_contrib_views that come before any launch (the
    pointers are never read)."""
    nat = pkg._native
    L = nat.lib()
    gv = pkg.torch_renderer.make_view(np.eye(4, dtype="float32"), np.eye(4, dtype="float32"), 50, 37, depth_grad=False)
    plan, empty = nat.GrPlan(1000, 0, 600), nat.GrPlan(0, 0, 0)
    need = L.gr_contrib_ws_bytes(ctypes.byref(gv), 10, ctypes.byref(plan))
    assert need >= 4 * 1000
    assert L.gr_contrib_ws_bytes(ctypes.byref(gv), 10, ctypes.byref(empty)) == 0
    assert L.gr_contrib_ws_bytes(ctypes.byref(gv), 0, ctypes.byref(plan)) == 0
    buf = (ctypes.c_float * 4)()
    p, null = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(0)

    def call(view=gv, n=10, pl=plan, geom=p, bins=p, saved=p, peak=p, ws=p, ws_bytes=need):
        return L.gr_contrib_view(ctypes.byref(view), n, ctypes.byref(pl), geom, bins, saved, peak, ws, ws_bytes, null)

    assert call(ws_bytes=need - 1) == nat.GR_ERR_WORKSPACE and b"workspace" in L.gr_last_error()
    for kw in (dict(geom=null), dict(bins=null), dict(saved=null), dict(peak=null), dict(ws=null)):
        assert call(**kw) == nat.GR_ERR_INVALID_ARGUMENT, kw
    for field, value in (("tile", 32), ("rows", 1), ("device_counts", 1)):
        bad = nat.GrView.from_buffer_copy(gv)
        setattr(bad, field, value)
        assert call(view=bad) == nat.GR_ERR_INVALID_ARGUMENT, field
    assert call(n=0) == nat.GR_OK and call(pl=empty, ws=null, ws_bytes=0) == nat.GR_OK  # no-ops: nothing is launched
    assert call(n=-1) == nat.GR_ERR_INVALID_ARGUMENT
    cfg = nat.GrFitConfig(1, 1, 1, 1, 0, 0)
    tgt = (nat.GrFitTarget * 1)()  # (null targets are fine)
    assert L.gr_contrib_views(null, ctypes.byref(cfg), 1, tgt, 10, p, p, p, 3, p, p, null) == nat.GR_ERR_INVALID_ARGUMENT
    assert L.gr_contrib_views(p, ctypes.byref(cfg), 1, tgt, 10, p, p, p, 3, p, null, null) == nat.GR_ERR_INVALID_ARGUMENT
    caps = (nat.GrPlan * 1)()
    cfg.caps = caps
    assert L.gr_contrib_views(p, ctypes.byref(cfg), 1, tgt, 10, p, p, p, 3, p, p, null) == nat.GR_ERR_INVALID_ARGUMENT
    assert b"caps" in L.gr_last_error()
    cfg.caps = None
    assert L.gr_contrib_views(p, ctypes.byref(cfg), 0, None, 10, p, p, p, 3, p, p, null) == nat.GR_OK  # no views
    assert L.gr_contrib_views(p, ctypes.byref(cfg), 1, tgt, 0, p, p, p, 3, p, p, null) == nat.GR_OK  # no Gaussians
    assert callable(pkg.torch_renderer.contrib_view_native)
    header = open(os.path.join(REPO, "include", "gr_hip.h")).read()
    assert "gr_contrib_view(" in header and "several streams may share one peak buffer" in header


def _main_args(tmp_path, *extra):
    return ["--targets_dir", os.path.join(GOLDEN, "fit_targets"), "--out_dir", str(tmp_path), "--iters", "6", "--width", str(W),
            "--height", str(H), "--num_gaussians", "150", "--seed", "1", "--device", "cpu", "--prune_interval", "3",
            "--densify_interval", "3", *extra]


def test_cli_prune_mode_contribution(fm, tmp_path, capsys):
    fm.main(_main_args(tmp_path / "c", "--prune_mode", "contribution", "--prune_contribution", "0.01"))
    out = capsys.readouterr().out
    assert out.count("prune at iter") == 2 and "peak blend weight of 150 Gaussians" in out and "opacity rule" in out
    for name in ("gaussians_fitted.npz", "loss.txt", "preview_view0.png"):
        assert (tmp_path / "c" / name).exists(), name
    assert len((tmp_path / "c" / "loss.txt").read_text().split()) == 6
    # the default mode prints no report and is the run without the flag
    fm.main(_main_args(tmp_path / "a"))
    fm.main(_main_args(tmp_path / "b", "--prune_mode", "opacity"))
    assert "prune at iter" not in capsys.readouterr().out
    for name in ("gaussians_fitted.npz", "loss.txt", "preview_view0.png"):
        assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes(), name
