"""The reference of the D-SSIM tests (tests/test_ssim_gpu.py, tests/test_ssim_cpu.py), their inputs and shapes.

The reference is a torch evaluation of the definition in include/gr_hip.h with a dense 121-tap conv2d (no separable
pass), in float64 on the float32-rounded inputs; its gradient comes from autograd.  The same evaluation in float32
gives e32, the error a plain float32 implementation has on an input, which sets the gradient tolerance.  Every
(kind, shape) is evaluated once per session and shared (lru_cache); callers must not modify what they get.
"""
from __future__ import annotations

import functools

import torch

TILE = 16  # GR_SSIM_TILE (include/gr_hip.h); test_ssim_gpu.py asserts the library's constant equals it

# (H, W, C): the smallest image; smaller than the window in both axes; exactly the window; one off the tile edge both
# ways; several tiles with overhang at four channels; a general multi-tile case
SHAPES = [(1, 1, 3), (5, 7, 3), (11, 11, 1), (TILE - 1, TILE + 1, 3), (TILE + 1, TILE - 1, 3), (2 * TILE + 3, TILE, 4),
          (64, 48, 3)]
KINDS = ["uniform", "render"]
GRAD_SCALE = 3.0  # the tests differentiate GRAD_SCALE * loss

VALUE_TOL = 2e-6  # |dssim - ref|: the L1 loss test's bar


def window(dtype) -> torch.Tensor:
    g = torch.exp(-(torch.arange(11, dtype=torch.float64) - 5.0) ** 2 / (2.0 * 1.5 ** 2))
    g = g / g.sum()
    return torch.outer(g, g).to(dtype)


def dssim_dense(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """1 - mean SSIM of (H, W, C) images in their own dtype: dense 11x11 window, zero padding of 5."""
    C = x.shape[2]
    w = window(x.dtype).expand(C, 1, 11, 11).contiguous()

    def conv(t):
        return torch.nn.functional.conv2d(t, w, padding=5, groups=C)

    X, Y = x.permute(2, 0, 1)[None], y.permute(2, 0, 1)[None]
    mx, my = conv(X), conv(Y)
    sx, sy, sxy = conv(X * X) - mx * mx, conv(Y * Y) - my * my, conv(X * Y) - mx * my
    m = ((2 * mx * my + 1e-4) * (2 * sxy + 9e-4)) / ((mx * mx + my * my + 1e-4) * (sx + sy + 9e-4))
    return 1.0 - m.mean()


def _blobs(H: int, W: int, C: int, gen: torch.Generator, centres=None):
    """A few smooth blobs on black, clamped to [0, 1]; returns the image and the blob centres."""
    k = 4
    if centres is None:
        centres = torch.rand((k, 2), generator=gen)
    amp = 0.4 + 0.9 * torch.rand((k, C), generator=gen)
    sig = 0.08 + 0.12 * torch.rand((k,), generator=gen)
    yy = (torch.arange(H, dtype=torch.float32) + 0.5)[:, None] / max(H, W)
    xx = (torch.arange(W, dtype=torch.float32) + 0.5)[None, :] / max(H, W)
    img = torch.zeros((H, W, C))
    for j in range(k):
        cy, cx = centres[j, 0] * H / max(H, W), centres[j, 1] * W / max(H, W)
        img += torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sig[j] ** 2))[..., None] * amp[j]
    return img.clamp(0.0, 1.0), centres


@functools.lru_cache(maxsize=None)
def inputs(kind: str, shape: tuple):
    """float32 CPU (x, y).  uniform: independent uniform noise.  render: blobs on a black background (flat regions),
    y's blobs slightly moved and re-coloured, the top half of y copied from x (equal regions): where
    conv(x^2) - mx^2 cancels."""
    H, W, C = shape
    gen = torch.Generator().manual_seed(1000 * H + 10 * W + C + (0 if kind == "uniform" else 7))
    if kind == "uniform":
        return torch.rand(shape, generator=gen), torch.rand(shape, generator=gen)
    x, centres = _blobs(H, W, C, gen)
    y, _ = _blobs(H, W, C, gen, centres + 0.03 * torch.randn(centres.shape, generator=gen))
    y[: H // 2] = x[: H // 2]
    return x.contiguous(), y.contiguous()


def _evaluate(x32, y32, dtype):
    x = x32.detach().clone().to(dtype).requires_grad_(True)  # (a copy: the cached inputs stay plain tensors)
    loss = dssim_dense(x, y32.to(dtype))
    (g,) = torch.autograd.grad(GRAD_SCALE * loss, x)
    return loss.detach(), g


@functools.lru_cache(maxsize=None)
def reference(kind: str, shape: tuple) -> dict:
    """loss (float64), grad of GRAD_SCALE * loss (float64), gmax = max|grad|, e32 = the float32 dense evaluation's
    max-abs gradient error against it, v32 its value error."""
    x, y = inputs(kind, shape)
    loss, g = _evaluate(x, y, torch.float64)
    loss32, g32 = _evaluate(x, y, torch.float32)
    return {"loss": float(loss), "grad": g, "gmax": float(g.abs().max()),
            "e32": float((g32.double() - g).abs().max()), "v32": abs(float(loss32) - float(loss))}


def grad_bound(ref: dict) -> float:
    """4 e32 (a separable two-pass float32 sum against a dense one: another summation order), at least 2e-6 max|g|."""
    return max(4.0 * ref["e32"], 2e-6 * ref["gmax"])
