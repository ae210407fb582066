"""Float64 dense restatement of one view's loss with exposure compensation and its gradients (helper of
test_exposure_*.py, not collected).

The view loss of the fit (fit_multiview_stub.py:292-305) with the photometric term on the exposed colour:

    x = clamp((bg + C) / (1 + W), 0, 1)                         the rendered colour, as everywhere else
    y = x @ E[:, :3].T + E[:, 3]                                E the view's 3 x 4 exposure matrix (not clamped)
    loss = (1 - l) mean|y - target| + l dssim(y, target) + w_sil mean|alpha - mask|
           + w_depth mean|depth / (max(depth) + 1e-6) - target_depth|        (l = w_dssim, 0 by default;
                                                                             dssim: tests/ssim_reference.dssim_dense)

evaluated in float64 torch from the three pixel sums (W, C, D) with tests/camera_reference.py's finalize (_images);
autograd (abs' = sign, sign(0) = 0; clamp passes the gradient on its closed interval) gives the gradients of
g_scale x loss to E and to the exposed image's inputs (the out / alpha / depth images: what a render backward takes to
reach the Gaussians).  The sums come from camera_reference.render, the dense float64 render (every Gaussian at every
pixel).
"""
from __future__ import annotations

import importlib

import numpy as np
import torch

import camera_reference as cref
import ssim_reference as sref
from oracle import oracle as orc

F = torch.float64


def _cv(t):
    return None if t is None else torch.as_tensor(t).detach().to("cpu", F)


def dense_sums(means, scales, colors, opacities, view, proj, W, H, background=None):
    """(Wt (H, W), C (H, W, 3), D (H, W)) float64 of camera_reference's dense render."""
    return cref.render(means, scales, colors, opacities, view, proj, W, H, background)[3:]


def exposed(sums, background, E):
    """(y, out, alpha, depth) float64, no gradient: the exposed colour and the images it is made from."""
    Wt, C, D = (_cv(t) for t in sums)
    bg = torch.zeros(3, dtype=F) if background is None else _cv(background)
    out, alpha, depth = cref._images(Wt, C, D, bg)
    E = _cv(E).reshape(3, 4)
    return out @ E[:, :3].T + E[:, 3], out, alpha, depth


def view_loss(sums, background, E, target, mask=None, w_sil=0.0, target_depth=None, w_depth=0.0, g_scale=1.0,
              w_dssim=0.0) -> dict:
    """loss (float, unscaled), and of g_scale x loss: dE (3, 4), g_out (H, W, 3), g_alpha (H, W) or None, g_depth
    (H, W) or None, all float64; margin = min|y - target| over all values (the kink's distance: a float32 evaluation
    within that of y has every sign right)."""
    Wt, C, D = (_cv(t) for t in sums)
    bg = torch.zeros(3, dtype=F) if background is None else _cv(background)
    out, alpha, depth = (t.clone().requires_grad_(True) for t in cref._images(Wt, C, D, bg))
    Et = _cv(E).reshape(3, 4).clone().requires_grad_(True)
    y = out @ Et[:, :3].T + Et[:, 3]
    loss = (y - _cv(target)).abs().mean()
    if w_dssim > 0.0:
        loss = (1.0 - w_dssim) * loss + w_dssim * sref.dssim_dense(y, _cv(target))
    ins = [Et, out]
    if mask is not None:
        loss = loss + w_sil * (alpha - _cv(mask)).abs().mean()
        ins.append(alpha)
    if target_depth is not None:
        loss = loss + w_depth * (depth / (depth.max() + 1e-6) - _cv(target_depth)).abs().mean()
        ins.append(depth)
    gs = list(torch.autograd.grad(g_scale * loss, ins))
    res = {"loss": float(loss.detach()), "dE": gs.pop(0), "g_out": gs.pop(0), "g_alpha": None, "g_depth": None,
           "margin": float((y.detach() - _cv(target)).abs().min())}
    if mask is not None:
        res["g_alpha"] = gs.pop(0)
    if target_depth is not None:
        res["g_depth"] = gs.pop(0)
    return res


def clear_targets(y, target, gap=1e-3, push=0.01):
    """`target` (float32 tensor like y) with the values closer than `gap` to the float64 y moved to y + push: the loss's
    kinks then lie at least ~gap from every value."""
    t = target.clone()
    near = (y - t.to(F)).abs() < gap
    t[near] = (y[near] + push).to(t.dtype)
    return t


# ---- the scenes shared by test_exposure_cpu.py and test_exposure_gpu.py --------------------------------------------------
W, H, V, N = 32, 24, 4, 80
RECOVERY_STEPS = 80


def exact_params(scene, device):
    """The fitter's raw parameters whose activations give the scene's own values (softplus + 1e-3, sigmoid)."""
    means, scales, colors, opac = (torch.from_numpy(a).double() for a in scene)
    inv_sig = lambda y: torch.log(y) - torch.log1p(-y)  # noqa: E731
    s = scales - 1e-3
    raw = {"means": means, "scales_raw": s + torch.log(-torch.expm1(-s)), "opacities_raw": inv_sig(opac),
           "colors_raw": inv_sig(colors)}
    return {k: torch.nn.Parameter(v.to(torch.float32).to(device)) for k, v in raw.items()}


def exposure_error(E, E_true) -> float:
    return float((E.double() - E_true.double()).abs().mean())


def scene_arrays(seed: int):
    rng = np.random.default_rng(seed)
    means = ((rng.random((N, 3)) - 0.5) * 1.2).astype(np.float32)
    scales = (rng.random((N, 3)) * 0.12 + 0.06).astype(np.float32)
    colors = (0.05 + 0.9 * rng.random((N, 3))).astype(np.float32)
    opac = (rng.random(N) * 0.5 + 0.3).astype(np.float32)
    return means, scales, colors, opac


def true_exposures(seed: int, signed: bool = False) -> torch.Tensor:
    """(V, 3, 4) float32: view 0 at identity, the others with gains about 0.8 .. 1.2, small off-diagonal terms and
    offsets about +-0.03.  signed: diagonal only, every row's offset with the sign of gain - 1, so that the residual
    x_k - (gain x_k + offset) of a render at identity exposure keeps one sign per row and stays at least 0.02 from
    zero wherever x lies in [0, 1] (a scene on which two renders that differ slightly take the same signs: no value sits near the loss's kink)."""
    rng = np.random.default_rng(seed)
    E = np.zeros((V, 3, 4), np.float64)
    for v in range(V):
        up = rng.random(3) < 0.5
        gain = np.where(up, 1.1 + 0.1 * rng.random(3), 0.9 - 0.1 * rng.random(3))
        off = 0.02 + 0.02 * rng.random(3)
        if signed:
            off = np.where(up, off, -off)
        else:
            off = off * np.where(rng.random(3) < 0.5, 1.0, -1.0)
            E[v, :, :3] = 0.02 * rng.standard_normal((3, 3))
        E[v, np.arange(3), np.arange(3)] = gain
        E[v, :, 3] = off
    E[0] = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    return torch.from_numpy(E).to(torch.float32)


def recovery_fitter(fm, device, signed: bool = False, **kw):
    """Targets rendered (dense, float64) from known Gaussians under known per-view exposures; the Gaussians start at
    truth and stay (lr = 0), the exposures start at identity, view 0 is at identity and fixed."""
    tr = importlib.import_module("3dgaussian_amd.torch_renderer")
    scene = scene_arrays(5)
    E_true = true_exposures(6, signed)
    cams = orc.orbit_cameras(V, W, H)
    targets = []
    for i, (view, proj) in enumerate(cams):
        y = exposed(dense_sums(*scene, view, proj, W, H), None, E_true[i])[0]
        targets.append(y.to(torch.float32).to(device))
    fc = [tr.Camera(view=torch.from_numpy(np.asarray(v, np.float32)).to(device),
                    proj=torch.from_numpy(np.asarray(p, np.float32)).to(device)) for v, p in cams]
    opts = dict(lr=0.0, masks=None, reg_opacity=0.0, reg_scale=0.0, exposure=True, exposure_lr=5e-3, exposure_fixed=(0,))
    opts.update(kw)
    fit = fm.ViewShardedFitter(exact_params(scene, device), fc, targets, W, H, **opts)
    return fit, E_true
