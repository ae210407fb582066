"""CPU: the construction rules of ViewShardedFitter(exposure_fused=True) and the CLI's --exposure_fused (the opt-in to
the HIP device's exposure form), which need no device: it requires exposure, it has no D-SSIM form, and on host tensors
it is accepted and changes nothing."""
from __future__ import annotations

import importlib
import os
import sys

import pytest
import torch

from conftest import GOLDEN

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import exposure_reference as eref  # noqa: E402

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


def test_requires_exposure(fm):
    params, cams, targets, masks = _small_setup(fm)
    with pytest.raises(ValueError, match="exposure_fused without exposure"):
        fm.ViewShardedFitter(params, cams, targets, W, H, masks=masks, exposure_fused=True)


def test_has_no_dssim_form(fm):
    params, cams, targets, masks = _small_setup(fm)
    with pytest.raises(ValueError, match="D-SSIM"):
        fm.ViewShardedFitter(params, cams, targets, W, H, masks=masks, exposure=True, exposure_fused=True, dssim_weight=0.2)
    with pytest.raises(ValueError, match="dssim_fused"):  # (the older rule keeps its text)
        fm.ViewShardedFitter(params, cams, targets, W, H, masks=masks, exposure=True, exposure_fused=True, dssim_weight=0.2,
                             dssim_fused=True)


def test_on_host_tensors_it_changes_nothing(fm):
    runs = []
    for kw in ({"exposure": True}, {"exposure": True, "exposure_fused": True}):
        params, cams, targets, masks = _small_setup(fm)
        fit = fm.ViewShardedFitter(params, cams, targets, W, H, masks=masks, exposure_fixed=(), **kw)
        fit.set_exposures(eref.true_exposures(2))
        losses = [fit.step().clone() for _ in range(3)]
        runs.append((losses, {k: v.detach().clone() for k, v in fit.params.items()}, fit.exposure_state()))
    assert runs[1][2][1].abs().max() > 0
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b)
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
    assert torch.equal(runs[0][2][0], runs[1][2][0]) and torch.equal(runs[0][2][1], runs[1][2][1])


def _main_args(out, *extra):
    return ["--targets_dir", os.path.join(GOLDEN, "fit_targets"), "--out_dir", str(out), "--iters", "2", "--width", "32",
            "--height", "24", "--num_gaussians", "40", "--seed", "1", "--device", "cpu", *extra]


def test_cli_flag(fm, tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        fm.main(_main_args(tmp_path / "bad", "--exposure_fused"))
    assert e.value.code == 2 and "--exposure_fused requires --exposure" in capsys.readouterr().err
    assert not (tmp_path / "bad").exists()
    fm.main(_main_args(tmp_path / "ok", "--exposure", "--exposure_fused"))
    assert (tmp_path / "ok" / "exposures.npz").exists()
    with pytest.raises(SystemExit):
        fm.main(["--help"])
    assert "--exposure_fused" in capsys.readouterr().out
