"""CPU: per-view exposure compensation in the fit (ViewShardedFitter(exposure=True), the CLI's --exposure) on host
tensors, where d loss / d E comes from autograd through view_loss, against the float64 restatement
tests/exposure_reference.py; off is off; identity on fixed views; validation; the CLI's exposures.npz; recovery of
known per-view exposures."""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import exposure_reference as eref  # noqa: E402
from exposure_reference import (RECOVERY_STEPS, exact_params, exposure_error, recovery_fitter, scene_arrays,  # noqa: E402
                                true_exposures)

GRAD_TOL = 1e-4  # the project's gradient bar (tests/test_camera_grad.py's CAM_TOL): relative L2
W, H, V = eref.W, eref.H, eref.V


@pytest.fixture(scope="module")
def fm():
    return importlib.import_module("3dgaussian_amd.fit_multiview")


def _small_setup(fm, n=60):
    torch.manual_seed(7)
    dev = torch.device("cpu")
    params = fm.build_params(n, dev, use_sh=False)
    with torch.no_grad():
        params["scales_raw"].fill_(-1.5)
    cams = fm.orbit_cameras(V, W, H, dev)
    g = torch.Generator().manual_seed(3)
    targets = [torch.rand((H, W, 3), generator=g) for _ in range(V)]
    masks = [(t.mean(2) > 0.5).float() for t in targets]
    return params, cams, targets, masks


# ---- the gradient against the float64 reference -----------------------------------------------------------------------
@pytest.mark.parametrize("form", ["l1", "depth", "dssim"])
def test_autograd_gradient_matches_the_reference(fm, form):
    """One step on host tensors with a non-trivial E per view: exposure_state()'s gradient against
    exposure_reference.view_loss on the dense float64 sums (targets kept 1e-3 from the kinks: the float32 render's
    signs are the reference's).  dssim: the exposed image reaches the D-SSIM term too."""
    tr = importlib.import_module("3dgaussian_amd.torch_renderer")
    scene = scene_arrays(1)
    cams = orc.orbit_cameras(V, W, H)
    E = true_exposures(2)
    E[0, 0, 1], E[0, 2, 3] = 0.05, -0.04  # (view 0 too)
    g = torch.Generator().manual_seed(4)
    sums = [eref.dense_sums(*scene, view, proj, W, H) for view, proj in cams]
    targets = [eref.clear_targets(eref.exposed(sums[i], None, E[i])[0], torch.rand((H, W, 3), generator=g)) for i in range(V)]
    masks = [(t.mean(2) > 0.5).float() for t in targets]
    depths = [torch.rand((H, W), generator=g) for _ in range(V)] if form == "depth" else None
    fc = [tr.Camera(view=torch.from_numpy(np.asarray(v, np.float32)), proj=torch.from_numpy(np.asarray(p, np.float32)))
          for v, p in cams]
    kw = {"dssim_weight": 0.3} if form == "dssim" else {}
    fit = fm.ViewShardedFitter(exact_params(scene, torch.device("cpu")), fc, targets, W, H, lr=0.0, masks=masks,
                               depths=depths, exposure=True, exposure_fixed=(), **kw)
    fit.set_exposures(E)
    loss = float(fit.step())
    E1, dE = fit.exposure_state()
    assert E1.shape == (V, 3, 4) and dE.shape == (V, 3, 4) and E1.dtype == torch.float32 and not dE.is_cuda
    refs = [eref.view_loss(sums[i], None, E[i], targets[i], masks[i], fit.w_sil, None if depths is None else depths[i],
                           fit.w_depth, 1.0 / V, fit.w_dssim) for i in range(V)]
    assert min(r["margin"] for r in refs) > 1e-4
    want = torch.stack([r["dE"] for r in refs])
    rel = float((dE.double() - want).norm() / want.norm())
    reg = float(fit.reg_opacity * torch.sigmoid(fit.params["opacities_raw"].detach()).mean()
                + fit.reg_scale * (torch.nn.functional.softplus(fit.params["scales_raw"].detach()) + 1e-3).mean())
    lref = sum(r["loss"] for r in refs) / V + reg
    print(f"{form}: host fitter d loss / d E vs the float64 reference: relL2 {rel:.2e}; loss {loss:.7f} reference {lref:.7f}")
    assert float(want.norm()) > 0 and rel <= GRAD_TOL
    assert abs(loss - lref) <= 2e-6
    # Adam's first step (bias-corrected moments g and g^2): exposure_lr against the gradient's sign
    assert torch.allclose(E1, E - 1e-3 * dE / (dE.abs() + 1e-8), rtol=0, atol=5e-7)


# ---- off is off, identity, validation ----------------------------------------------------------------------------------
def test_off_is_off(fm):
    runs = []
    for kw in ({}, {"exposure": False}):
        params, cams, targets, masks = _small_setup(fm)
        fit = fm.ViewShardedFitter(params, cams, targets, W, H, masks=masks, **kw)
        losses = [fit.step().clone() for _ in range(3)]
        runs.append((losses, {k: v.detach().clone() for k, v in fit.params.items()}, fit))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b)
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
    with pytest.raises(ValueError, match="exposure"):
        runs[1][2].exposure_state()
    assert runs[1][2].exposure is False


def test_identity_on_fixed_views_is_off(fm):
    runs = []
    for kw in ({}, {"exposure": True, "exposure_fixed": tuple(range(V))}):
        params, cams, targets, masks = _small_setup(fm)
        fit = fm.ViewShardedFitter(params, cams, targets, W, H, masks=masks, **kw)
        runs.append(([fit.step().clone() for _ in range(3)], fit))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b)
    E, dE = runs[1][1].exposure_state()
    eye = torch.cat([torch.eye(3), torch.zeros(3, 1)], dim=1)
    assert all(torch.equal(E[v], eye) for v in range(V)) and not dE.any()


def test_validation(fm):
    params, cams, targets, masks = _small_setup(fm)
    with pytest.raises(ValueError, match="dssim_fused"):
        fm.ViewShardedFitter(params, cams, targets, W, H, masks=masks, exposure=True, dssim_weight=0.2, dssim_fused=True)
    for bad in ((V,), (-1,), (0, V + 3)):
        with pytest.raises(ValueError, match="exposure_fixed"):
            fm.ViewShardedFitter(params, cams, targets, W, H, masks=masks, exposure=True, exposure_fixed=bad)
    fit = fm.ViewShardedFitter(params, cams, targets, W, H, masks=masks, exposure=True, exposure_fixed=(2, 1, 1))
    assert fit.exposure_fixed == (1, 2)
    fit.step()
    E, dE = fit.exposure_state()
    eye = torch.cat([torch.eye(3), torch.zeros(3, 1)], dim=1)
    assert torch.equal(E[1], eye) and torch.equal(E[2], eye) and not dE[1].any() and not dE[2].any()
    assert not torch.equal(E[0], eye) and not torch.equal(E[3], eye) and float(dE[0].abs().min()) > 0


def test_set_exposures_resumes_a_fit(fm, tmp_path):
    """exposure_state() / exposures.npz fed back through set_exposures: the next step starts from those matrices."""
    params, cams, targets, masks = _small_setup(fm)
    fit = fm.ViewShardedFitter(params, cams, targets, W, H, masks=masks, exposure=True, exposure_fixed=())
    E = true_exposures(3)
    np.savez(tmp_path / "exposures.npz", exposure=E.numpy())
    with np.load(tmp_path / "exposures.npz") as d:
        fit.set_exposures(d["exposure"])
    assert torch.equal(fit.exposure_state()[0], E)
    fit.step()
    E1, dE = fit.exposure_state()
    assert float((E1 - E).abs().max()) <= 1e-3 * 1.01 and float((E1 - E).abs().min()) > 0 and dE.abs().min() > 0
    with pytest.raises(ValueError, match="shape"):
        fit.set_exposures(E[:2])
    plain = fm.ViewShardedFitter(*_small_setup(fm)[:3], W, H)
    with pytest.raises(ValueError, match="exposure"):
        plain.set_exposures(E)


def test_densify_and_evaluate_leave_the_exposures_alone(fm):
    params, cams, targets, masks = _small_setup(fm)
    fit = fm.ViewShardedFitter(params, cams, targets, W, H, masks=masks, exposure=True)
    fit.step()
    opt, E = fit._expo_opt, fit.exposure_state()[0]
    a = fit.evaluate()  # the metric is of the image rendered from the Gaussians: no exposure, whatever E is
    fit.set_exposures(3.0 * E)
    b = fit.evaluate()
    fit.set_exposures(E)
    assert np.array_equal(a["l1"], b["l1"]) and np.array_equal(a["psnr"], b["psnr"]) and np.array_equal(a["ssim"], b["ssim"])
    m, s, c, o = fm.activations(fit.params)
    with torch.no_grad():
        l1 = float((fit.render_fn(m, s, c, o, fit.cams[1], W, H, fit._background(m.device))[0] - targets[1]).abs().mean())
    assert abs(float(a["l1"][1]) - l1) <= 1e-6
    fit.densify_and_prune(max_gaussians=80, densify_ratio=0.2, prune_opacity=0.05)
    fit.reset_optimizer()
    fit.respatialize()
    assert fit._expo_opt is opt and torch.equal(fit.exposure_state()[0], E) and len(opt.state) == 1
    fit.step()
    assert not torch.equal(fit.exposure_state()[0], E)


# ---- recovery ---------------------------------------------------------------------------------------------------------
def test_recovery(fm):
    fit, E_true = recovery_fitter(fm, torch.device("cpu"))
    e0 = exposure_error(fit.exposure_state()[0], E_true)
    before = {k: v.detach().clone() for k, v in fit.params.items()}
    for _ in range(RECOVERY_STEPS):
        fit.step()
    E = fit.exposure_state()[0]
    e1 = exposure_error(E, E_true)
    print(f"mean |E - E_true| {e0:.5f} -> {e1:.5f} (ratio {e1 / e0:.3f}) after {RECOVERY_STEPS} steps")
    assert all(torch.equal(before[k], fit.params[k].detach()) for k in before)  # lr = 0: the Gaussians stay exact
    assert torch.equal(E[0], E_true[0])  # the fixed view
    assert e1 <= 0.5 * e0


# ---- the CLI ------------------------------------------------------------------------------------------------------------
def _main_args(out, *extra):
    return ["--targets_dir", os.path.join(GOLDEN, "fit_targets"), "--out_dir", str(out), "--iters", "3", "--width", "32",
            "--height", "24", "--num_gaussians", "40", "--seed", "1", "--device", "cpu", *extra]


def test_cli_writes_the_exposures(fm, tmp_path):
    plain, ex, held = tmp_path / "plain", tmp_path / "ex", tmp_path / "held"
    fm.main(_main_args(plain))
    assert not (plain / "exposures.npz").exists()
    fm.main(_main_args(ex, "--exposure", "--exposure_lr", "2e-3"))
    with np.load(ex / "exposures.npz") as d:
        E = d["exposure"]
    eye = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(np.float32)
    assert E.shape == (3, 3, 4) and E.dtype == np.float32
    assert np.array_equal(E[0], eye)  # --exposure_fix 0 (the default)
    assert not np.array_equal(E[1], eye) and not np.array_equal(E[2], eye)
    assert np.abs(E - eye).max() <= 3 * 2e-3 * 1.01  # three Adam steps at most lr each
    # the training views only, in their order; no fixed view: every exposure moves; held-out metrics are written
    fm.main(_main_args(held, "--exposure", "--exposure_fix", "none", "--holdout_every", "3"))
    with np.load(held / "exposures.npz") as d:
        assert d["exposure"].shape == (2, 3, 4) and not np.array_equal(d["exposure"][0], eye)
    assert (held / "eval.json").exists()
    with pytest.raises(ValueError, match="exposure_fixed"):
        fm.main(_main_args(tmp_path / "bad", "--exposure", "--exposure_fix", "7"))
    import contextlib
    import io
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), pytest.raises(SystemExit):
        fm.main(["--help"])
    assert "without exposure" in " ".join(buf.getvalue().split())
