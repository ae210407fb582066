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


def _one_step(fm, cuda, setup, lam, fused, direct=True, native=None, depth=False):
    """(loss, gradients, updated parameters, view_loss calls, (_direct, _graph_ok)) of a fresh fitter's first step;
    masks on and no depth term, or with `depth` a depth term and no masks."""
    bench = importlib.import_module("bench")
    cams, targets, masks, depths = setup
    saved = fm.DIRECT_BACKWARD, fm.NATIVE_EXEC
    fm.DIRECT_BACKWARD = direct
    if native is not None:
        fm.NATIVE_EXEC = native
    try:
        f = fm.ViewShardedFitter(bench.synthetic_params(N, cuda), cams, targets, W, H, masks=None if depth else masks,
                                 depths=depths if depth else None, dssim_weight=lam, dssim_fused=fused)
        calls = []
        inner = f.view_loss
        f.view_loss = lambda *a, **kw: (calls.append(a[0]), inner(*a, **kw))[1]
        flags = f._direct(cuda), f._graph_ok(cuda)
        loss = f.step().detach().clone()
        torch.cuda.synchronize()
        grads = {k: v.grad.detach().clone() for k, v in f.params.items()}
        params = {k: v.detach().clone() for k, v in f.params.items()}
    finally:
        fm.DIRECT_BACKWARD, fm.NATIVE_EXEC = saved
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


@pytest.mark.parametrize("depth", [False, True], ids=["masks", "depth"])
def test_executor_matches_python_schedule(fm, cuda, setup, depth):
    """The native executor's D-SSIM form against the Python schedule, bit for bit and run to run; with masks, and
    with a depth term and no masks."""
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
