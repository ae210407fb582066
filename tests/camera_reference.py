"""Float64 dense restatement of one view's camera gradient (helper of test_camera_refine_*.py, not collected).

The render of the reference (python/torch_renderer.py:109-203: projection, sigma rule, RGB / SH colour with the view
direction through inv(view), weights, out / alpha / depth) written out in float64 torch with the camera's `view` and
`proj` as leaf tensors, so that autograd gives d view, d proj of
L = <out, g_out> + <alpha, g_alpha> + <depth, g_depth> for upstream gradient images g_*.  No tiles and no footprint
cutoff: every Gaussian at every pixel.

L depends on the camera only through the three pixel sums (W, C, D), so the images' gradients w.r.t. those sums are
taken first and the Gaussians then go through in chunks (memory O(chunk x H x W)), as tests/density_reference.py does.
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


def _sh3_tail(d):
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz = x * x, y * y, z * z
    return torch.stack([x * y, y * z, 3.0 * zz - 1.0, x * z, xx - yy, y * (3.0 * xx - yy), x * y * z,
                        y * (5.0 * zz - 1.0), z * (5.0 * zz - 3.0), x * (5.0 * zz - 1.0), z * (xx - yy),
                        x * (xx - 3.0 * yy)], dim=1)


def _colors(colors, means, view):
    if colors.ndim == 2:
        return colors
    cam = torch.linalg.inv(view)[:3, 3]
    d = cam.view(1, 3) - means
    d = d / (torch.linalg.norm(d, dim=1, keepdim=True) + 1e-8)
    out = colors[:, 0, :] + colors[:, 1, :] * d[:, 0:1] + colors[:, 2, :] * d[:, 1:2] + colors[:, 3, :] * d[:, 2:3]
    if colors.shape[1] == 16:
        out = out + torch.einsum("nb,nbc->nc", _sh3_tail(d), colors[:, 4:, :])
    return out


def _gaussians(means, scales, colors, opacities, view, proj, W, H):
    """Per Gaussian: px, py, sx, sy, opacity x valid, clamped colour, z_abs (functions of view and proj)."""
    px, py, valid, za = _project(means, view, proj, W, H)
    fx, fy = proj[0, 0].abs(), proj[1, 1].abs()
    sx = (scales[:, 0].abs() * 0.5 * W * fx / za).clamp_min(1.0)
    sy = (scales[:, 1].abs() * 0.5 * H * fy / za).clamp_min(1.0)
    ov = opacities.clamp_min(0.0) * valid.to(F)
    col = _colors(colors, means, view).clamp(0.0, 1.0)
    return px, py, sx, sy, ov, col, za


def _weights(px, py, sx, sy, ov, W, H):
    dx = (torch.arange(W, dtype=F) + 0.5)[None, :] - px[:, None]
    dy = (torch.arange(H, dtype=F) + 0.5)[None, :] - py[:, None]
    ex = torch.exp(-0.5 * dx * dx / (sx * sx)[:, None])
    ey = torch.exp(-0.5 * dy * dy / (sy * sy)[:, None])
    return ov[:, None, None] * ey[:, :, None] * ex[:, None, :]


def _cv(t):
    return None if t is None else torch.as_tensor(t).detach().to("cpu", F)


def render(means, scales, colors, opacities, view, proj, W, H, background=None, chunk=128):
    """(out, alpha, depth) of the dense render in float64, no gradient."""
    means, scales, colors, opacities, view, proj = (_cv(t) for t in (means, scales, colors, opacities, view, proj))
    bg = torch.zeros(3, dtype=F) if background is None else _cv(background)
    with torch.no_grad():
        px, py, sx, sy, ov, col, za = _gaussians(means, scales, colors, opacities, view, proj, W, H)
        Wt, C, D = torch.zeros((H, W), dtype=F), torch.zeros((H, W, 3), dtype=F), torch.zeros((H, W), dtype=F)
        for a in range(0, means.shape[0], chunk):
            s = slice(a, a + chunk)
            w = _weights(px[s], py[s], sx[s], sy[s], ov[s], W, H)
            Wt += w.sum(0)
            C += torch.einsum("ghw,gc->hwc", w, col[s])
            D += torch.einsum("ghw,g->hw", w, za[s])
    return _images(Wt, C, D, bg) + (Wt, C, D)


def _images(Wt, C, D, bg):
    out = ((bg.view(1, 1, 3) + C) / (1.0 + Wt)[..., None]).clamp(0.0, 1.0)
    alpha = (Wt / (1.0 + Wt)).clamp(0.0, 1.0)
    depth = (D / (Wt + 1e-6)).clamp_min(0.0)
    return out, alpha, depth


def camera_grads(means, scales, colors, opacities, view, proj, W, H, g_out, g_alpha=None, g_depth=None,
                 background=None, chunk=128):
    """(d view, d proj) (4, 4) float64 of L = <out, g_out> + <alpha, g_alpha> + <depth, g_depth>, and the dense
    (out, alpha, depth).  colors: (N, 3) RGB, (N, 4, 3) or (N, 16, 3) SH.  Inputs of any float dtype / device."""
    means, scales, colors, opacities = (_cv(t) for t in (means, scales, colors, opacities))
    g_out, g_alpha, g_depth = _cv(g_out), _cv(g_alpha), _cv(g_depth)
    bg = torch.zeros(3, dtype=F) if background is None else _cv(background)
    out, alpha, depth, Wt, C, D = render(means, scales, colors, opacities, view, proj, W, H, bg, chunk)
    Wt, C, D = (t.clone().requires_grad_(True) for t in (Wt, C, D))
    o2, a2, d2 = _images(Wt, C, D, bg)
    L = (o2 * g_out).sum()
    if g_alpha is not None:
        L = L + (a2 * g_alpha).sum()
    if g_depth is not None:
        L = L + (d2 * g_depth).sum()
    gW, gC, gD = torch.autograd.grad(L, (Wt, C, D), allow_unused=True)
    gW = torch.zeros((H, W), dtype=F) if gW is None else gW
    gD = torch.zeros((H, W), dtype=F) if gD is None else gD
    vt = _cv(view).clone().requires_grad_(True)  # the leaves
    pt = _cv(proj).clone().requires_grad_(True)
    dview, dproj = torch.zeros((4, 4), dtype=F), torch.zeros((4, 4), dtype=F)
    for a in range(0, means.shape[0], chunk):
        s = slice(a, a + chunk)
        px, py, sx, sy, ov, col, za = _gaussians(means[s], scales[s], colors[s], opacities[s], vt, pt, W, H)
        w = _weights(px, py, sx, sy, ov, W, H)
        per = gW[None] + torch.einsum("hwc,gc->ghw", gC, col) + gD[None] * za[:, None, None]
        dv, dp = torch.autograd.grad((w * per).sum(), (vt, pt))
        dview += dv
        dproj += dp
    return dview, dproj, out, alpha, depth
