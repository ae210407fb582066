"""GPU: the fused D-SSIM loss (3dgaussian_amd/losses.py dssim_loss / ssim, gr_ssim_* in libgr_hip.so) against the
float64 dense-window reference of tests/ssim_reference.py, and its wiring into ViewShardedFitter (dssim_weight).

Gradient error of the kernels, max|g - g_ref| / max|g_ref| per shape, beside the float32 dense torch evaluation's
(e32 / max|g_ref|): profiles/ssim_loss.txt.
"""
from __future__ import annotations

import ctypes
import importlib

import pytest
import torch

import ssim_reference as sr

pytestmark = pytest.mark.gpu

CASES = [(k, s) for k in sr.KINDS for s in sr.SHAPES]
IDS = [f"{k}-{'x'.join(map(str, s))}" for k, s in CASES]


@pytest.fixture(scope="module")
def losses(pkg):
    return importlib.import_module("3dgaussian_amd.losses")


def test_tile_constant(pkg):
    assert pkg._native.SSIM_TILE == sr.TILE


@pytest.mark.parametrize("kind,shape", CASES, ids=IDS)
def test_value(losses, cuda, kind, shape):
    x, y = (t.to(cuda) for t in sr.inputs(kind, shape))
    ref = sr.reference(kind, shape)
    got = float(losses.dssim_loss(x, y))
    print(f"ssim value {kind} {shape}: err {abs(got - ref['loss']):.3e} (float32 dense torch {ref['v32']:.3e})")
    assert abs(got - ref["loss"]) <= sr.VALUE_TOL


@pytest.mark.parametrize("kind,shape", CASES, ids=IDS)
def test_gradient(losses, cuda, kind, shape):
    x, y = (t.to(cuda) for t in sr.inputs(kind, shape))
    ref = sr.reference(kind, shape)
    pred = x.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(sr.GRAD_SCALE * losses.dssim_loss(pred, y), pred)
    err = float((g.double().cpu() - ref["grad"]).abs().max())
    bound = sr.grad_bound(ref)
    gm = ref["gmax"]
    print(f"ssim grad {kind} {shape}: err/gmax {err / gm:.3e} e32/gmax {ref['e32'] / gm:.3e} bound/gmax {bound / gm:.3e}")
    assert g.shape == x.shape and torch.isfinite(g).all()
    assert err <= bound


@pytest.mark.parametrize("kind,shape", [("uniform", (64, 48, 3)), ("render", (2 * sr.TILE + 3, sr.TILE, 4)),
                                        ("uniform", (5, 7, 3))])
def test_ssim_metric(losses, cuda, kind, shape):
    a, b = (t.to(cuda) for t in sr.inputs(kind, shape))
    s = losses.ssim(a, b)
    assert s.dim() == 0 and not s.requires_grad
    assert abs(float(s) - (1.0 - float(losses.dssim_loss(a, b)))) <= 1e-6
    assert float(losses.ssim(a, a)) >= 1.0 - 1e-6
    # a metric: no graph even when the input wants a gradient
    assert not losses.ssim(a.clone().requires_grad_(True), b).requires_grad


def test_deterministic(losses, cuda):
    x, y = (t.to(cuda) for t in sr.inputs("uniform", (64, 48, 3)))
    out = []
    for _ in range(2):
        pred = x.clone().requires_grad_(True)
        loss = losses.dssim_loss(pred, y)
        (g,) = torch.autograd.grad(sr.GRAD_SCALE * loss, pred)
        out.append((loss.detach().clone(), g.clone()))
    assert torch.equal(out[0][0], out[1][0])
    assert torch.equal(out[0][1], out[1][1])


def test_errors(pkg, losses, cuda):
    a = torch.zeros((8, 9, 3), device=cuda)
    with pytest.raises(ValueError):
        losses.dssim_loss(a, torch.zeros((8, 9, 4), device=cuda))
    with pytest.raises(ValueError):
        losses.ssim(a, torch.zeros((9, 8, 3), device=cuda))
    nat = pkg._native
    L = nat.lib()
    for want in (0, 1):
        need = int(L.gr_ssim_ws_bytes(8, 9, 3, want))
        ws = torch.zeros((need,), dtype=torch.uint8, device=cuda)
        out = torch.zeros((), device=cuda)
        st = L.gr_ssim_fwd(nat.ptr(a), nat.ptr(a), 8, 9, 3, want, nat.ptr(out), nat.ptr(ws), need - 1, ctypes.c_void_p(0))
        assert st == nat.GR_ERR_WORKSPACE and b"workspace" in L.gr_last_error()
    g = torch.ones((), device=cuda)
    st = L.gr_ssim_bwd(nat.ptr(a), nat.ptr(a), 8, 9, 3, nat.ptr(g), nat.ptr(ws), need - 1, nat.ptr(torch.empty_like(a)),
                       ctypes.c_void_p(0))
    assert st == nat.GR_ERR_WORKSPACE and b"workspace" in L.gr_last_error()


def _scene(fm, dev, n=40, W=48, H=40, n_views=3):
    """tests/test_fit_dp.py::_setup, on the device."""
    torch.manual_seed(7)
    params = fm.build_params(n, dev, use_sh=False)
    with torch.no_grad():
        params["scales_raw"].fill_(-1.0)
    cams = fm.orbit_cameras(n_views, W, H, dev)
    g = torch.Generator().manual_seed(3)
    targets = [torch.rand((H, W, 3), generator=g).to(dev) for _ in range(n_views)]
    return params, cams, targets, W, H


def _step_against_manual(fm, losses, dev, lam):
    """Per parameter: (max|fitter grad - manual grad|, max|manual grad|) after one step(); the view_loss calls."""
    params, cams, targets, W, H = _scene(fm, dev)
    fit = fm.ViewShardedFitter(params, cams, targets, W, H, masks=None, dssim_weight=lam)
    start = {k: v.detach().clone().requires_grad_(True) for k, v in fit.params.items()}  # (the fitter's Morton order)
    calls = []
    inner = fit.view_loss
    fit.view_loss = lambda *a, **kw: (calls.append(a[0]), inner(*a, **kw))[1]
    direct = fit._direct(dev)
    loss = fit.step()
    torch.cuda.synchronize()
    got = {k: v.grad.detach().clone() for k, v in fit.params.items()}
    # the same loss through public ops only
    means, scales, colors, opacities = fm.activations(start)
    total = 0.0
    for cam, tgt in zip(cams, targets):
        pred, _, _ = fm.hip_render(means, scales, colors, opacities, cam, W, H, torch.zeros(3, device=dev), depth_grad=False)
        total = total + (1.0 - lam) * losses.l1_loss(pred, tgt) + lam * losses.dssim_loss(pred, tgt)
    manual = total / len(targets) + fit.reg_opacity * opacities.mean() + fit.reg_scale * scales.mean()
    manual.backward()
    torch.cuda.synchronize()
    diff = {k: (float((got[k] - start[k].grad).abs().max()), float(start[k].grad.abs().max())) for k in got}
    return diff, calls, direct, float(loss), float(manual)


def test_fitter_wiring(pkg, losses, cuda):
    """dssim_weight = 0.2: one step() leaves the gradient of (1 - l) L1 + l D-SSIM (+ regulariser) composed from public
    ops, up to accumulation order across streams.  Margin: the same comparison at dssim_weight = 0 (the fit as it
    was), times 4, at least 1e-6 max|grad|."""
    fm = importlib.import_module("3dgaussian_amd.fit_multiview")
    base, _, _, _, _ = _step_against_manual(fm, losses, cuda, 0.0)
    diff, calls, direct, loss, manual = _step_against_manual(fm, losses, cuda, 0.2)
    assert not direct  # l > 0: not the fused path ...
    assert sorted(calls) == [0, 1, 2]  # ... but the per-view autograd path, every view once
    assert abs(loss - manual) <= 1e-6 * max(1.0, abs(manual))
    for k, (d, gmax) in diff.items():
        bound = max(4.0 * base[k][0], 1e-6 * gmax)
        print(f"fitter wiring {k}: diff {d:.3e} (l = 0: {base[k][0]:.3e}) max|grad| {gmax:.3e} bound {bound:.3e}")
        assert gmax > 0.0 and d <= bound
