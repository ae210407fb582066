"""GPU: ViewShardedFitter's exposure argument on the HIP device.  The fused fit path has no exposure form yet, so
exposure=True raises there (no quiet fall-back to the per-view autograd path), and exposure=False leaves every path's
losses and parameters bit-identical to a fitter built without the argument."""
from __future__ import annotations

import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

FW, FH, FN, FV = 64, 48, 300, 6


def _fit_scene(cuda):
    fm = importlib.import_module("3dgaussian_amd.fit_multiview")
    cams = fm.orbit_cameras(FV, FW, FH, cuda)
    g = torch.Generator(device=cuda).manual_seed(21)
    targets = [torch.rand((FH, FW, 3), generator=g, device=cuda) for _ in range(FV)]
    masks = [(t.mean(dim=2) > 0.5).float() for t in targets]
    return fm, cams, targets, masks


def test_exposure_raises_on_the_hip_device(cuda):
    fm, cams, targets, masks = _fit_scene(cuda)
    bench = importlib.import_module("bench")
    with pytest.raises(ValueError, match="HIP device"):
        fm.ViewShardedFitter(bench.synthetic_params(FN, cuda), cams, targets, FW, FH, masks=masks, exposure=True)


@pytest.mark.parametrize("mode", ["0", "batch"])
def test_off_is_off(cuda, mode):
    fm, cams, targets, masks = _fit_scene(cuda)
    bench = importlib.import_module("bench")
    saved = fm.GRAPH_MODE
    runs = []
    try:
        fm.GRAPH_MODE = mode
        for kw in ({}, {"exposure": False}):
            f = fm.ViewShardedFitter(bench.synthetic_params(FN, cuda), cams, targets, FW, FH, masks=masks, **kw)
            losses = [f.step().clone() for _ in range(3)]
            f.graph_sync()
            runs.append((losses, {k: v.detach().clone() for k, v in f.params.items()}))
    finally:
        fm.GRAPH_MODE = saved
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
    assert all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1])
