"""Float64 dense reference of the blend-weighted pixel error per Gaussian (helper of test_error_*.py, not collected).

On tests/camera_reference.py's restatement of the reference render (``_gaussians``, ``_weights``, ``render``): every
Gaussian at every pixel, no tiles and no footprint cutoff.  With out = clamp((bg + C) / (1 + Wt)) the rendered image,
e(p) = mean_k |out_k(p) - target_k(p)|, r(p) = 1 / (1 + Wt(p)) and b_i(p) = w_i(p) r(p) the blend weights,

    ref[i] = sum_p b_i(p) e(p),    B[i] = sum_p b_i(p),    S = sum_p r(p) e(p).

sum_i b_i + r = 1 at every pixel, so sum_i ref[i] + S = sum_p e(p): the view's L1 error partitioned among the
Gaussians and the background.  Scenes: contribution_reference.scene (its DEAD Gaussians come out exactly 0).

Tolerance of a tiled float32 evaluation (``tolerance``): |got - ref| <= 1e-4 ref + delta B + o exp(-cutoff^2 / 2) S.
The first term is the project's parity bar for rendered sums.  delta bounds the evaluation's error of e per pixel: the
largest absolute difference between the float32 image the statistic is formed from and the float64 image (the mean of
three channels' absolute differences moves by at most the largest of them), measured by the caller on the existing
render; weighted by b it sums to at most delta B.  The last term is exact: a pixel outside a Gaussian's kept tiles
has w < o exp(-cutoff^2 / 2), and it is left out with weight r(p) e(p), e <= 1.
"""
from __future__ import annotations

import math

import torch

import camera_reference as cref
from contribution_reference import DEAD, scene  # noqa: F401  (the tests' scenes)

F = torch.float64


def error_ref(means, scales, colors, opacities, view, proj, W, H, target, background=None, exposure=None, chunk=64):
    """(ref (N,), B (N,), S, out (H, W, 3), Wt (H, W)) float64 for one view.  ``exposure`` ((3, 4)): e compares
    E (out, 1) with the target; ``out`` is returned without it."""
    means, scales, colors, opacities, view, proj, target = (cref._cv(t) for t in (means, scales, colors, opacities, view,
                                                                                   proj, target))
    n = means.shape[0]
    with torch.no_grad():
        px, py, sx, sy, ov, _, _ = cref._gaussians(means, scales, colors, opacities, view, proj, W, H)
        res = cref.render(means, scales, colors, opacities, view, proj, W, H, background)
        out, Wt = res[0], res[3]
        x = out
        if exposure is not None:
            E = cref._cv(exposure)
            x = out @ E[:, :3].t() + E[:, 3]
        e = (x - target).abs().sum(-1) / 3.0
        r = 1.0 / (1.0 + Wt)
        ref, B = torch.zeros((n,), dtype=F), torch.zeros((n,), dtype=F)
        for a in range(0, n, chunk):
            s = slice(a, a + chunk)
            b = cref._weights(px[s], py[s], sx[s], sy[s], ov[s], W, H) * r[None]
            ref[s] = (b * e[None]).flatten(1).sum(dim=1)
            B[s] = b.flatten(1).sum(dim=1)
    return ref, B, float((r * e).sum()), out, Wt


def error_ref_views(means, scales, colors, opacities, cams, W, H, targets, background=None):
    """(max over the views of ref, of B, of S): the per-view tolerance terms are each bounded by their maxima."""
    n = means.shape[0]
    ref, B, S = torch.zeros((n,), dtype=F), torch.zeros((n,), dtype=F), 0.0
    for (view, proj), t in zip(cams, targets):
        r1, b1, s1, _, _ = error_ref(means, scales, colors, opacities, view, proj, W, H, t, background)
        ref, B, S = torch.maximum(ref, r1), torch.maximum(B, b1), max(S, s1)
    return ref, B, S


def tolerance(ref, B, S, opacities, cutoff, delta):
    return 1e-4 * ref + delta * B + cref._cv(opacities).clamp_min(0.0) * math.exp(-0.5 * cutoff * cutoff) * S


def worst_ratio(got, ref, tol):
    """max_i |got - ref| / tolerance (0 / 0 counts as 0): <= 1 passes."""
    err = (cref._cv(got) - ref).abs()
    ratio = torch.where(err > 0, err / tol.clamp_min(1e-300), torch.zeros_like(err))
    return float(ratio.max()) if ratio.numel() else 0.0
