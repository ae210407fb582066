"""Float64 dense restatement of one view's loss with per-pixel loss weights and its gradients (helper of
test_weights_*.py, not collected).

The view loss of the fit (fit_multiview_stub.py:292-305) with every L1 term of pixel p counted w_p >= 0 times:

    loss = (1 / (3 HW)) sum_p w_p sum_k |out_pk - t_pk| + w_sil (1 / HW) sum_p w_p |alpha_p - m_p|
           + w_depth (1 / HW) sum_p w_p |depth_p / (M + 1e-6) - td_p|,      M = max_p depth_p  (all pixels, unweighted)

evaluated in float64 torch from the three pixel sums (W, C, D) with tests/camera_reference.py's finalize (_images), as
exposure_reference.view_loss is; autograd (abs' = sign, sign(0) = 0; max shares its gradient evenly among ties) gives
the gradients of g_scale x loss to the out / alpha / depth images.  fit_loss_and_grads differentiates the same loss
through camera_reference's dense render (every Gaussian at every pixel) down to the fitter's raw parameters.
"""
from __future__ import annotations

import numpy as np
import torch

import camera_reference as cref
from exposure_reference import _cv, clear_targets, dense_sums  # noqa: F401  (re-exported for the tests)

F = torch.float64


def weighted_loss(out, alpha, depth, weight, target, mask=None, w_sil=0.0, target_depth=None, w_depth=0.0):
    """The loss above from float64 images (differentiable)."""
    w = _cv(weight)
    loss = (w[..., None] * (out - _cv(target)).abs()).mean()
    if mask is not None:
        loss = loss + w_sil * (w * (alpha - _cv(mask)).abs()).mean()
    if target_depth is not None:
        loss = loss + w_depth * (w * (depth / (depth.max() + 1e-6) - _cv(target_depth)).abs()).mean()
    return loss


def view_loss(sums, background, weight, target, mask=None, w_sil=0.0, target_depth=None, w_depth=0.0, g_scale=1.0) -> dict:
    """loss (float, unscaled), and of g_scale x loss: g_out (H, W, 3), g_alpha (H, W) or None, g_depth (H, W) or None,
    all float64; margin = min|out - target| over the values with a positive weight (the kink's distance)."""
    Wt, C, D = (_cv(t) for t in sums)
    bg = torch.zeros(3, dtype=F) if background is None else _cv(background)
    out, alpha, depth = (t.clone().requires_grad_(True) for t in cref._images(Wt, C, D, bg))
    loss = weighted_loss(out, alpha, depth, weight, target, mask, w_sil, target_depth, w_depth)
    ins = [out] + ([alpha] if mask is not None else []) + ([depth] if target_depth is not None else [])
    gs = list(torch.autograd.grad(g_scale * loss, ins))
    seen = _cv(weight) > 0
    res = {"loss": float(loss.detach()), "g_out": gs.pop(0), "g_alpha": None, "g_depth": None,
           "margin": float((out.detach() - _cv(target)).abs()[seen].min())}
    if mask is not None:
        res["g_alpha"] = gs.pop(0)
    if target_depth is not None:
        res["g_depth"] = gs.pop(0)
    return res


def dense_images(means, scales, colors, opacities, view, proj, W, H, background=None):
    """(out, alpha, depth) of camera_reference's dense render, differentiable in the four (float64) parameter tensors."""
    view, proj = _cv(view), _cv(proj)
    bg = torch.zeros(3, dtype=F) if background is None else _cv(background)
    px, py, sx, sy, ov, col, za = cref._gaussians(means, scales, colors, opacities, view, proj, W, H)
    w = cref._weights(px, py, sx, sy, ov, W, H)
    Wt = w.sum(0)
    C = torch.einsum("ghw,gc->hwc", w, col)
    D = torch.einsum("ghw,g->hw", w, za)
    return cref._images(Wt, C, D, bg)


def fit_loss_and_grads(raw: dict, cams, W, H, weights, targets, masks=None, w_sil=0.0, depths=None, w_depth=0.0,
                       reg_opacity=0.0, reg_scale=0.0) -> tuple:
    """The fit step's loss in float64 from the fitter's raw parameters (softplus + 1e-3, sigmoid): the mean of the views'
    weighted losses plus the regulariser; returns (per-view losses, total loss, {name: d total / d raw})."""
    leaves = {k: _cv(v).clone().requires_grad_(True) for k, v in raw.items()}
    means = leaves["means"]
    scales = torch.nn.functional.softplus(leaves["scales_raw"]) + 1e-3
    colors = torch.sigmoid(leaves["colors_raw"])
    opac = torch.sigmoid(leaves["opacities_raw"])
    per = []
    for i, (view, proj) in enumerate(cams):
        out, alpha, depth = dense_images(means, scales, colors, opac, view, proj, W, H)
        per.append(weighted_loss(out, alpha, depth, weights[i], targets[i], None if masks is None else masks[i], w_sil,
                                 None if depths is None else depths[i], w_depth))
    total = sum(per) / len(per) + reg_opacity * opac.mean() + reg_scale * scales.mean()
    names = list(leaves)
    grads = torch.autograd.grad(total, [leaves[k] for k in names])
    return [float(p.detach()) for p in per], float(total.detach()), dict(zip(names, grads))


# the GPU tests' zero rectangles (x0, y0, x1, y1) per view size: at 50 x 37 (4 x 3 tiles of 16 pixels) all of tile (1, 1)
# and part of its eight neighbours, 480 of 1,850 pixels; at 16 x 16 and 7 x 5 part of the only tile
GPU_RECTS = {(50, 37): (12, 13, 36, 33), (16, 16): (4, 4, 12, 12), (7, 5): (2, 1, 5, 4)}
GPU_WEIGHT_SEED = 5


def weight_map(W: int, H: int, rect, seed: int = 0) -> torch.Tensor:
    """(H, W) float32 weights, random in [0.25, 4] with the rectangle rect = (x0, y0, x1, y1) (half-open) at zero."""
    rng = np.random.default_rng(seed)
    w = (0.25 + 3.75 * rng.random((H, W))).astype(np.float32)
    x0, y0, x1, y1 = rect
    w[y0:y1, x0:x1] = 0.0
    return torch.from_numpy(w)


def tile_cover(w: torch.Tensor, tile: int = 16) -> dict:
    """Per tile (ty, tx) of the map: (in-image pixels, those with a positive weight)."""
    H, W = w.shape
    out = {}
    for ty in range(-(-H // tile)):
        for tx in range(-(-W // tile)):
            blk = w[ty * tile:(ty + 1) * tile, tx * tile:(tx + 1) * tile]
            out[(ty, tx)] = (blk.numel(), int((blk > 0).sum()))
    return out
