"""Float64 dense reference of the peak blend weight per Gaussian (helper of test_contribution_*.py, not collected).

On tests/camera_reference.py's restatement of the reference render (``_gaussians``, ``_weights`` and ``render``'s weight
sum ``Wt``): every Gaussian at every pixel, no tiles and no footprint cutoff,

    peak_ref[i] = max_p w_i(p) / (1 + Wt(p)).

Removing Gaussian i changes pixel p by w (out - c_i) / (1 + Wt - w), at most b / (1 - b) in every channel with
b = w / (1 + Wt), because out and c_i lie in [0, 1] (``removal_change`` evaluates the left side exactly).

Tolerance of a tiled float32 evaluation against it (``tolerance``): |got - ref| <= 1e-4 ref + o exp(-cutoff^2 / 2).  The
first term is the project's parity bar for rendered sums; the second is exact: a pixel outside a Gaussian's kept tiles
has w < o exp(-cutoff^2 / 2), and b <= w.
"""
from __future__ import annotations

import math

import torch

import camera_reference as cref

F = torch.float64
DEAD = 4  # Gaussians appended to every scene whose peak is exactly 0


def scene(n, seed=0, sigma=0.05, spread=0.6):
    """n random Gaussians around the origin and DEAD more of which no orbit camera of the fit loop (radius 2.5,
    elevation 0.2, looking at the origin, fovy 60) sees a trace: one behind the camera (high above: behind every orbit
    position's image plane), one fully off screen (far below: in front of every position, 74 degrees off its axis),
    one with opacity 0 and one with negative opacity.  (means, scales, colors, opacities) float32 on the host; the
    last DEAD rows are the dead ones."""
    g = torch.Generator().manual_seed(seed)
    means = (torch.rand((n, 3), generator=g) - 0.5) * 2.0 * spread
    scales = sigma * (0.5 + torch.rand((n, 3), generator=g))
    colors = torch.rand((n, 3), generator=g)
    opac = 0.05 + 0.95 * torch.rand((n,), generator=g)
    dead_m = torch.tensor([[0.0, 30.0, 0.0], [0.0, -30.0, 0.0], [0.05, 0.0, 0.0], [-0.05, 0.05, 0.0]])
    dead_s = torch.full((DEAD, 3), 0.03)
    dead_o = torch.tensor([0.9, 0.9, 0.0, -0.5])
    return (torch.cat([means, dead_m]).contiguous(), torch.cat([scales, dead_s]).contiguous(),
            torch.cat([colors, torch.full((DEAD, 3), 0.5)]).contiguous(), torch.cat([opac, dead_o]).contiguous())


def peak_ref(means, scales, opacities, view, proj, W, H, chunk=64):
    """(peak (N,), Wt (H, W)) float64: the dense definition for one view."""
    means, scales, opacities, view, proj = (cref._cv(t) for t in (means, scales, opacities, view, proj))
    n = means.shape[0]
    colors = torch.zeros((n, 3), dtype=F)
    with torch.no_grad():
        px, py, sx, sy, ov, _, _ = cref._gaussians(means, scales, colors, opacities, view, proj, W, H)
        Wt = cref.render(means, scales, colors, opacities, view, proj, W, H)[3]
        r = 1.0 / (1.0 + Wt)
        peak = torch.zeros((n,), dtype=F)
        for a in range(0, n, chunk):
            s = slice(a, a + chunk)
            w = cref._weights(px[s], py[s], sx[s], sy[s], ov[s], W, H)
            peak[s] = (w * r[None]).flatten(1).max(dim=1).values
    return peak, Wt


def peak_ref_views(means, scales, opacities, cams, W, H):
    """The maximum of peak_ref over (view, proj) pairs."""
    out = torch.zeros((means.shape[0],), dtype=F)
    for view, proj in cams:
        out = torch.maximum(out, peak_ref(means, scales, opacities, view, proj, W, H)[0])
    return out


def tolerance(ref, opacities, cutoff):
    return 1e-4 * ref + cref._cv(opacities).clamp_min(0.0) * math.exp(-0.5 * cutoff * cutoff)


def worst_ratio(got, ref, opacities, cutoff):
    """max_i |got - ref| / tolerance (0 / 0 counts as 0): <= 1 passes."""
    err = (cref._cv(got) - ref).abs()
    tol = tolerance(ref, opacities, cutoff)
    ratio = torch.where(err > 0, err / tol.clamp_min(1e-300), torch.zeros_like(err))
    return float(ratio.max()) if ratio.numel() else 0.0


def removal_change(means, scales, colors, opacities, view, proj, W, H, i, background=None):
    """max over pixels and channels of |render - render without Gaussian i|, dense float64."""
    keep = torch.ones(means.shape[0], dtype=torch.bool)
    keep[i] = False
    a = cref.render(means, scales, colors, opacities, view, proj, W, H, background)[0]
    b = cref.render(means[keep], scales[keep], colors[keep], opacities[keep], view, proj, W, H, background)[0]
    return float((a - b).abs().max())
