"""CPU: the torch path of losses.dssim_loss / ssim on host tensors against the float64 dense-window reference
(tests/ssim_reference.py), the gr_ssim_* entry points' argument checks (no launch), and the dssim_weight option of
ViewShardedFitter and fit_multiview.main on host tensors."""
from __future__ import annotations

import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

import ssim_reference as sr
from conftest import GOLDEN

CASES = [("uniform", (64, 48, 3)), ("render", (2 * sr.TILE + 3, sr.TILE, 4))]


@pytest.fixture(scope="module")
def losses(pkg):
    return importlib.import_module("3dgaussian_amd.losses")


@pytest.fixture(scope="module")
def fm(pkg):
    return importlib.import_module("3dgaussian_amd.fit_multiview")


@pytest.mark.parametrize("kind,shape", CASES)
def test_cpu_path_value_and_gradient(losses, kind, shape):
    x, y = sr.inputs(kind, shape)
    ref = sr.reference(kind, shape)
    pred = x.clone().requires_grad_(True)
    loss = losses.dssim_loss(pred, y)
    (g,) = torch.autograd.grad(sr.GRAD_SCALE * loss, pred)
    loss = loss.detach()
    assert loss.dim() == 0 and abs(float(loss) - ref["loss"]) <= sr.VALUE_TOL
    assert float((g.double() - ref["grad"]).abs().max()) <= sr.grad_bound(ref)
    s = losses.ssim(x, y)
    assert not s.requires_grad and abs(float(s) - (1.0 - float(loss))) <= 1e-6
    assert float(losses.ssim(x, x)) >= 1.0 - 1e-6


def test_shape_mismatch_raises(losses):
    with pytest.raises(ValueError):
        losses.dssim_loss(torch.zeros((8, 9, 3)), torch.zeros((8, 9, 4)))
    with pytest.raises(ValueError):
        losses.ssim(torch.zeros((8, 9, 3)), torch.zeros((9, 8, 3)))
    with pytest.raises(ValueError):
        losses.dssim_loss(torch.zeros((8, 9, 5)), torch.zeros((8, 9, 5)))
    assert {"dssim_loss", "ssim", "l1_loss"} <= set(losses.__all__)


def test_abi_rejects_bad_arguments(pkg):
    """The three entry points load and validate before any launch: the pointers here are never dereferenced."""
    nat = pkg._native
    L = nat.lib()
    buf = (ctypes.c_float * 4)()
    p, null = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(0)
    assert L.gr_ssim_ws_bytes(40, 48, 3, 0) > 0
    assert L.gr_ssim_ws_bytes(40, 48, 3, 1) >= L.gr_ssim_ws_bytes(40, 48, 3, 0) + 3 * 40 * 48 * 3 * 4
    big = 1 << 40
    bad_shapes = [(0, 48, 3), (40, 0, 3), (-1, 48, 3), (40, 48, 0), (40, 48, 5)]
    for h, w, c in bad_shapes:
        assert L.gr_ssim_fwd(p, p, h, w, c, 1, p, p, big, null) == nat.GR_ERR_INVALID_ARGUMENT
        assert L.gr_last_error()
        assert L.gr_ssim_bwd(p, p, h, w, c, p, p, big, p, null) == nat.GR_ERR_INVALID_ARGUMENT
    for args in ((null, p, 40, 48, 3, 1, p, p, big, null), (p, null, 40, 48, 3, 1, p, p, big, null),
                 (p, p, 40, 48, 3, 1, null, p, big, null), (p, p, 40, 48, 3, 1, p, null, big, null)):
        assert L.gr_ssim_fwd(*args) == nat.GR_ERR_INVALID_ARGUMENT
    for args in ((null, p, 40, 48, 3, p, p, big, p, null), (p, p, 40, 48, 3, null, p, big, p, null),
                 (p, p, 40, 48, 3, p, null, big, p, null), (p, p, 40, 48, 3, p, p, big, null, null)):
        assert L.gr_ssim_bwd(*args) == nat.GR_ERR_INVALID_ARGUMENT
    need = L.gr_ssim_ws_bytes(40, 48, 3, 1)
    assert L.gr_ssim_fwd(p, p, 40, 48, 3, 1, p, p, need - 1, null) == nat.GR_ERR_WORKSPACE
    assert b"workspace" in L.gr_last_error()
    assert L.gr_ssim_bwd(p, p, 40, 48, 3, p, p, need - 1, p, null) == nat.GR_ERR_WORKSPACE
    with pytest.raises(ValueError):
        nat.check(L.gr_ssim_fwd(p, p, 40, 48, 5, 0, p, p, big, null), "gr_ssim_fwd")


def _scene(fm, n_views=2, n=40, W=24, H=20):
    torch.manual_seed(7)
    dev = torch.device("cpu")
    params = fm.build_params(n, dev, use_sh=False)
    with torch.no_grad():
        params["scales_raw"].fill_(-1.0)
    cams = fm.orbit_cameras(n_views, W, H, dev)
    return params, cams, W, H


def _clone(params):
    return {k: torch.nn.Parameter(v.detach().clone()) for k, v in params.items()}


def _render(fm, params, cam, W, H):
    with torch.no_grad():
        return fm.hip_render(*fm.activations(params), cam, W, H, torch.zeros(3))[0]


def test_zero_weight_is_the_fit_as_it_was(fm):
    params, cams, W, H = _scene(fm)
    g = torch.Generator().manual_seed(3)
    targets = [torch.rand((H, W, 3), generator=g) for _ in cams]
    masks = [(t.mean(2) > 0.5).float() for t in targets]
    a = fm.ViewShardedFitter(_clone(params), cams, targets, W, H, masks=masks)
    b = fm.ViewShardedFitter(_clone(params), cams, targets, W, H, masks=masks, dssim_weight=0.0)
    for _ in range(2):
        assert torch.equal(a.step(), b.step())
    for k in a.params:
        assert torch.equal(a.params[k].detach(), b.params[k].detach())
    with pytest.raises(ValueError):
        fm.ViewShardedFitter(_clone(params), cams, targets, W, H, dssim_weight=1.5)


def test_fit_with_dssim_term_lowers_dssim(fm, losses):
    """Targets rendered from the scene, the fit started from a perturbed copy: 30 steps of (1 - l) L1 + l D-SSIM lower
    view 0's D-SSIM."""
    params, cams, W, H = _scene(fm)
    with torch.no_grad():
        params["colors_raw"].add_(1.5)  # visible colours (the initial ones are near black)
    targets = [_render(fm, params, cam, W, H) for cam in cams]
    start = _clone(params)
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        start["means"].add_(0.08 * torch.randn(start["means"].shape, generator=gen))
        start["colors_raw"].add_(0.8 * torch.randn(start["colors_raw"].shape, generator=gen))
    fit = fm.ViewShardedFitter(start, cams, targets, W, H, masks=None, dssim_weight=0.2)
    assert not fit._direct(torch.device("cpu"))
    before = float(losses.dssim_loss(_render(fm, fit.params, cams[0], W, H), targets[0]))
    first = float(fit.step())
    for _ in range(29):
        last = float(fit.step())
    after = float(losses.dssim_loss(_render(fm, fit.params, cams[0], W, H), targets[0]))
    print(f"dssim of view 0: {before:.5f} -> {after:.5f}; loss {first:.5f} -> {last:.5f}")
    assert before > 0.0 and after < before


def test_main_with_dssim_weight_on_cpu(fm, tmp_path):
    fm.main(["--targets_dir", os.path.join(GOLDEN, "fit_targets"), "--out_dir", str(tmp_path), "--iters", "2",
             "--width", "32", "--height", "32", "--num_gaussians", "60", "--seed", "1", "--device", "cpu",
             "--dssim_weight", "0.2"])
    assert len((tmp_path / "loss.txt").read_text().split()) == 2
    with np.load(tmp_path / "gaussians_fitted.npz") as d:
        assert abs(float(d["dssim_weight"]) - 0.2) < 1e-7 and d["means"].shape == (60, 3)
