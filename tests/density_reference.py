"""Float64 dense restatement of one view's density statistic (helper of test_density_*.py, not collected).

The render of the reference (python/torch_renderer.py:109-203: projection, sigma rule, weights, out / alpha / depth)
written out in float64 torch with the Gaussians' pixel centres px, py as leaf tensors, so that autograd gives
d L / d px, d L / d py of L = <out, g_out> + <alpha, g_alpha> + <depth, g_depth> for upstream gradient images g_*.
The statistic is hypot(d px (W - 1) / 2, d py (H - 1) / 2): the gradient's norm w.r.t. the NDC position
(px = (ndc_x / 2 + 1 / 2)(W - 1)).  No tiles and no footprint cutoff: every Gaussian at every pixel.

L depends on the pixel centres only through the three pixel sums (W, C, D), linearly, so the images' gradients
w.r.t. those sums are taken first and the Gaussians then go through in chunks (memory O(chunk x H x W)).
"""
from __future__ import annotations

import torch

F = torch.float64


def _project(means, view, proj, W, H):
    n = means.shape[0]
    pc = torch.cat([means, torch.ones((n, 1), dtype=F)], dim=1) @ view.t()
    clip = pc @ proj.t()
    w = clip[:, 3]
    ws = torch.where(w.abs() < 1e-8, torch.ones_like(w), w)
    ndc = clip[:, :3] / ws[:, None]
    px = (ndc[:, 0] * 0.5 + 0.5) * (W - 1)
    py = (1.0 - (ndc[:, 1] * 0.5 + 0.5)) * (H - 1)
    valid = (ndc[:, 2] >= -1.0) & (ndc[:, 2] <= 1.0) & (w != 0.0)
    za = pc[:, 2].abs().clamp_min(1e-6)
    return px, py, valid, za


def _weights(px, py, sx, sy, ov, W, H):
    """(G, H, W): ov exp(-dx^2 / (2 sx^2)) exp(-dy^2 / (2 sy^2)) at the pixel centres x + 0.5, y + 0.5."""
    dx = (torch.arange(W, dtype=F) + 0.5)[None, :] - px[:, None]
    dy = (torch.arange(H, dtype=F) + 0.5)[None, :] - py[:, None]
    ex = torch.exp(-0.5 * dx * dx / (sx * sx)[:, None])
    ey = torch.exp(-0.5 * dy * dy / (sy * sy)[:, None])
    return ov[:, None, None] * ey[:, :, None] * ex[:, None, :]


def view_statistic(means, scales, colors, opacities, view, proj, W, H, g_out, g_alpha=None, g_depth=None,
                   background=None, chunk=128):
    """Per Gaussian: hypot(dL/dpx (W-1)/2, dL/dpy (H-1)/2) in float64, and (out, alpha) of the dense render.
    colors: (N, 3) RGB.  Inputs of any float dtype / device; computed on the CPU."""
    cv = lambda t: None if t is None else torch.as_tensor(t).detach().to("cpu", F)
    means, scales, colors, opacities, view, proj = (cv(t) for t in (means, scales, colors, opacities, view, proj))
    g_out, g_alpha, g_depth = cv(g_out), cv(g_alpha), cv(g_depth)
    bg = torch.zeros(3, dtype=F) if background is None else cv(background)
    assert colors.ndim == 2 and colors.shape[1] == 3
    n = means.shape[0]
    px, py, valid, za = _project(means, view, proj, W, H)
    fx, fy = proj[0, 0].abs(), proj[1, 1].abs()
    sx = (scales[:, 0].abs() * 0.5 * W * fx / za).clamp_min(1.0)
    sy = (scales[:, 1].abs() * 0.5 * H * fy / za).clamp_min(1.0)
    ov = opacities.clamp_min(0.0) * valid.to(F)
    col = colors.clamp(0.0, 1.0)
    Wt, C, D = torch.zeros((H, W), dtype=F), torch.zeros((H, W, 3), dtype=F), torch.zeros((H, W), dtype=F)
    for a in range(0, n, chunk):
        w = _weights(px[a:a + chunk], py[a:a + chunk], sx[a:a + chunk], sy[a:a + chunk], ov[a:a + chunk], W, H)
        Wt += w.sum(0)
        C += torch.einsum("ghw,gc->hwc", w, col[a:a + chunk])
        D += torch.einsum("ghw,g->hw", w, za[a:a + chunk])
    Wt.requires_grad_(True)
    C.requires_grad_(True)
    D.requires_grad_(True)
    out = ((bg.view(1, 1, 3) + C) / (1.0 + Wt)[..., None]).clamp(0.0, 1.0)
    alpha = (Wt / (1.0 + Wt)).clamp(0.0, 1.0)
    depth = (D / (Wt + 1e-6)).clamp_min(0.0)
    L = (out * g_out).sum()
    if g_alpha is not None:
        L = L + (alpha * g_alpha).sum()
    if g_depth is not None:
        L = L + (depth * g_depth).sum()
    gW, gC, gD = torch.autograd.grad(L, (Wt, C, D), allow_unused=True)
    gW = torch.zeros_like(Wt) if gW is None else gW
    gD = torch.zeros_like(D) if gD is None else gD
    stat = torch.empty(n, dtype=F)
    for a in range(0, n, chunk):
        pxa = px[a:a + chunk].clone().requires_grad_(True)  # the leaves
        pya = py[a:a + chunk].clone().requires_grad_(True)
        w = _weights(pxa, pya, sx[a:a + chunk], sy[a:a + chunk], ov[a:a + chunk], W, H)
        per = gW[None] + torch.einsum("hwc,gc->ghw", gC, col[a:a + chunk]) + gD[None] * za[a:a + chunk, None, None]
        dpx, dpy = torch.autograd.grad((w * per).sum(), (pxa, pya))
        stat[a:a + chunk] = torch.hypot(dpx * (0.5 * (W - 1)), dpy * (0.5 * (H - 1)))
    return stat, out.detach(), alpha.detach()


def l1_upstream(out, alpha, target, mask, w_sil, H, W):
    """The upstream images of the fit's view loss mean|out - target| + w_sil mean|alpha - mask| (unscaled), with the
    kink's signs taken from the given images (the caller passes the images whose gradient it compares with)."""
    cv = lambda t: torch.as_tensor(t).detach().to("cpu", F)
    g_out = torch.sign(cv(out) - cv(target)) / (3 * H * W)
    g_alpha = None
    if mask is not None and w_sil > 0.0:
        g_alpha = torch.sign(cv(alpha) - cv(mask)) * (w_sil / (H * W))
    return g_out, g_alpha
