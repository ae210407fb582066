"""GPU, fitter level: ViewShardedFitter(dssim_fused=True) takes the fused path's D-SSIM form (gr_bwd_fit_ssim_gather per
view through the Python schedule or the native executor) and agrees with the per-view autograd path."""
from __future__ import annotations

import importlib

import pytest
import torch

from test_ssim_gpu import _scene

pytestmark = pytest.mark.gpu

W, H, VIEWS, N, LAM = 96, 80, 6, 5000, 0.2


@pytest.fixture(scope="module")
def fm(pkg, cuda):
    return importlib.import_module("3dgaussian_amd.fit_multiview")


@pytest.fixture(scope="module")
def setup(fm, cuda):
    cams = fm.orbit_cameras(VIEWS, W, H, cuda)
    g = torch.Generator(device=cuda).manual_seed(9)
    targets = [torch.rand((H, W, 3), generator=g, device=cuda) for _ in cams]
    masks = [(t.mean(dim=2) > 0.5).float() for t in targets]
    depths = [torch.rand((H, W), generator=g, device=cuda) for _ in cams]
    return cams, targets, masks, depths


# 11 views of 64x48, 300 Gaussians, on 4 streams in reduction batches of 2 with a tail of 1 (a stream of three views
# reduces three times, the last a short tail) and preparation groups of 1, then 2, three views ahead (the groups run
# out mid-step), for two steps: the batch and tail bookkeeping of the Python schedule's loop
SMALL_BATCHES = dict(NUM_STREAMS=4, REDUCE_BATCH=2, REDUCE_TAIL=1, PREP_GROUP=2, PREP_FIRST=1, PREP_AHEAD=3)


@pytest.fixture(scope="module")
def setup_small(fm, cuda):
    w, h, views = 64, 48, 11
    cams = fm.orbit_cameras(views, w, h, cuda)
    g = torch.Generator(device=cuda).manual_seed(9)
    targets = [torch.rand((h, w, 3), generator=g, device=cuda) for _ in cams]
    masks = [(t.mean(dim=2) > 0.5).float() for t in targets]
    return cams, targets, masks, None


def _one_step(fm, cuda, setup, lam, fused, direct=True, native=None, depth=False, knobs=None, steps=1, n=N):
    """(loss, gradients, updated parameters, view_loss calls, (_direct, _graph_ok)) of a fresh fitter's first step (of
    its last of `steps`); masks on and no depth term, or with `depth` a depth term and no masks.  knobs: module
    switches of the schedule set for the run."""
    bench = importlib.import_module("bench")
    cams, targets, masks, depths = setup
    h, w = targets[0].shape[:2]
    saved = fm.DIRECT_BACKWARD, fm.NATIVE_EXEC
    saved_knobs = {k: getattr(fm, k) for k in (knobs or {})}
    fm.DIRECT_BACKWARD = direct
    if native is not None:
        fm.NATIVE_EXEC = native
    try:
        for k, v in (knobs or {}).items():
            setattr(fm, k, v)
        f = fm.ViewShardedFitter(bench.synthetic_params(n, cuda), cams, targets, w, h, masks=None if depth else masks,
                                 depths=depths if depth else None, dssim_weight=lam, dssim_fused=fused)
        calls = []
        inner = f.view_loss
        f.view_loss = lambda *a, **kw: (calls.append(a[0]), inner(*a, **kw))[1]
        flags = f._direct(cuda), f._graph_ok(cuda)
        for _ in range(steps):
            loss = f.step().detach().clone()
        torch.cuda.synchronize()
        grads = {k: v.grad.detach().clone() for k, v in f.params.items()}
        params = {k: v.detach().clone() for k, v in f.params.items()}
    finally:
        fm.DIRECT_BACKWARD, fm.NATIVE_EXEC = saved
        for k, v in saved_knobs.items():
            setattr(fm, k, v)
    return loss, grads, params, calls, flags


def test_path_selection(fm, cuda, setup):
    _, _, _, calls, (direct, graph) = _one_step(fm, cuda, setup, LAM, True)
    assert direct and not graph and calls == []
    _, _, _, calls, (direct, graph) = _one_step(fm, cuda, setup, LAM, False)
    assert not direct and not graph and sorted(calls) == list(range(VIEWS))  # exactly the path as it was


def test_step_matches_autograd_path(fm, cuda, setup):
    """One step, fused against unfused: the loss within 1e-6 relative, every gradient within max(4 e0, 1e-6) relative
    L2, e0 the same quantity of the L1 fit (l = 0) between its fused path and its autograd path: the two bin with
    different footprints (tests/test_fit_gpu.py::test_direct_path_matches_autograd_path), so the yardstick is measured."""
    la, ga, _, _, _ = _one_step(fm, cuda, setup, 0.0, False, direct=False)
    ld, gd, _, _, _ = _one_step(fm, cuda, setup, 0.0, False, direct=True)
    e0 = {k: float((gd[k] - ga[k]).norm() / ga[k].norm()) for k in ga}
    lu, gu, _, _, _ = _one_step(fm, cuda, setup, LAM, False)
    lf, gf, _, _, _ = _one_step(fm, cuda, setup, LAM, True)
    print(f"dssim fused fit: loss {float(lf):.7f} unfused {float(lu):.7f}")
    ok = abs(float(lf) - float(lu)) <= 1e-6 * abs(float(lu))
    for k in gu:
        err = float((gf[k] - gu[k]).norm() / gu[k].norm())
        print(f"  {k}: relL2 {err:.3e} (l = 0: {e0[k]:.3e})")
        ok = ok and err <= max(4.0 * e0[k], 1e-6)
    assert ok


@pytest.mark.parametrize("depth", [False, True, "small-batches"], ids=["masks", "depth", "small-batches"])
def test_executor_matches_python_schedule(fm, cuda, setup, setup_small, depth):
    """The native executor's D-SSIM form against the Python schedule, bit for bit and run to run; with masks, and
    with a depth term and no masks; and with masks at SMALL_BATCHES' knobs over two steps."""
    if depth == "small-batches":
        runs = [_one_step(fm, cuda, setup_small, LAM, True, native=nv, knobs=SMALL_BATCHES, steps=2, n=300)
                for nv in ("1", "1", "0", "0")]
    else:
        runs = [_one_step(fm, cuda, setup, LAM, True, native=nv, depth=depth) for nv in ("1", "1", "0", "0")]
    for r in runs:
        assert r[3] == [] and r[4][0]
    ref = runs[0]
    for r in runs[1:]:
        assert torch.equal(r[0], ref[0])
        for k in ref[1]:
            assert torch.equal(r[1][k], ref[1][k]), k
            assert torch.equal(r[2][k], ref[2][k]), k
    assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0.0 for g in ref[1].values())


def test_fused_fit_lowers_the_loss(fm, cuda):
    params, cams, targets, w, h = _scene(fm, cuda)
    f = fm.ViewShardedFitter(params, cams, targets, w, h, masks=None, dssim_weight=LAM, dssim_fused=True)
    assert f._direct(cuda)
    curve = [float(f.step()) for _ in range(20)]
    print(f"dssim fused fit: loss {curve[0]:.5f} -> {curve[-1]:.5f}")
    assert curve[-1] < curve[0]
