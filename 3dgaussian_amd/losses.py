"""Fused fit-loop losses on the HIP device (the caller's side of the render op).

``l1_loss(a, b, c=None, d=None, w2=0.0)`` = ``mean|a - b| + w2 * mean|c - d|``: the photometric L1
plus the weighted silhouette L1 of python/fit_multiview_stub.py:292-299, as one forward reduction
(k_l1_partial + k_l1_final) and one backward kernel (k_l1_grad) in libgr_hip.so instead of torch's
chain of sub / abs / mean / mul / add launches and their backward.  Same value and gradient as the
torch expression up to float32 summation order (tests/test_losses_gpu.py); deterministic.

``dssim_loss(pred, target)`` = ``1 - mean SSIM`` of two channel-last ``(H, W, C)`` images (11x11 Gaussian
window, sigma 1.5, zero padding, C1 = 1e-4, C2 = 9e-4; include/gr_hip.h), the structural term of
``(1 - l) * L1 + l * (1 - SSIM)``: one tiled forward kernel (k_ssim_fwd, separable windowed sums in LDS)
plus the final sum, and one backward kernel (k_ssim_bwd) over three maps the forward keeps, instead of
about ten conv2d and fifteen elementwise launches with their autograd graph.  ``ssim(a, b)`` is the
mean SSIM as a metric (no gradient, no maps).  On CPU tensors both evaluate the same definition with
torch ops, so that a ``--device cpu`` fit works (tests/test_ssim_gpu.py, tests/test_ssim_cpu.py).
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import torch

try:
    from . import _native
except ImportError:  # pragma: no cover
    import _native  # type: ignore


def _stream(t: torch.Tensor) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


class _L1Loss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, c, d, w2):
        L = _native.lib()
        n1 = a.numel()
        n2 = 0 if c is None else c.numel()
        loss = torch.empty((), dtype=torch.float32, device=a.device)
        ws = torch.empty((int(L.gr_l1_loss_ws_bytes()),), dtype=torch.uint8, device=a.device)
        _native.check(L.gr_l1_loss_fwd(_native.ptr(a), _native.ptr(b), n1, _native.ptr(c), _native.ptr(d), n2,
                                       ctypes.c_float(w2), _native.ptr(loss), _native.ptr(ws), ws.numel(), _stream(a)),
                      "gr_l1_loss_fwd")
        ctx.save_for_backward(a, b, c, d)
        ctx.w2 = w2
        return loss

    @staticmethod
    def backward(ctx, g):
        a, b, c, d = ctx.saved_tensors
        L = _native.lib()
        g = g.contiguous().float()
        ga = torch.empty_like(a)
        gc = None if c is None else torch.empty_like(c)
        _native.check(L.gr_l1_loss_bwd(_native.ptr(a), _native.ptr(b), a.numel(), _native.ptr(c), _native.ptr(d),
                                       0 if c is None else c.numel(), ctypes.c_float(ctx.w2), _native.ptr(g),
                                       _native.ptr(ga), _native.ptr(gc), _stream(a)), "gr_l1_loss_bwd")
        return ga, None, gc, None, None


def l1_loss(a: torch.Tensor, b: torch.Tensor, c: Optional[torch.Tensor] = None, d: Optional[torch.Tensor] = None,
            w2: float = 0.0) -> torch.Tensor:
    """mean|a - b| + w2 * mean|c - d| on the HIP device; gradients flow to a and c (the rendered
    image and alpha), not to the targets b and d."""
    if a.device.type != "cuda":
        raise RuntimeError("l1_loss runs on the HIP device; there is no CPU path")
    if a.shape != b.shape or (c is not None and (d is None or c.shape != d.shape)):
        raise ValueError("l1_loss: shape mismatch")
    f = lambda t: None if t is None else t.contiguous().float()  # noqa: E731
    return _L1Loss.apply(f(a), f(b).detach(), f(c), None if d is None else f(d).detach(), float(w2))


SSIM_WINDOW, SSIM_SIGMA, SSIM_C1, SSIM_C2 = 11, 1.5, 1e-4, 9e-4


def _ssim_map_torch(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """The SSIM map (1, C, H, W) of two (H, W, C) images with torch ops: the definition of include/gr_hip.h."""
    C = x.shape[2]
    r = SSIM_WINDOW // 2
    g = torch.exp(-(torch.arange(SSIM_WINDOW, dtype=torch.float64) - r) ** 2 / (2.0 * SSIM_SIGMA ** 2))
    g = g / g.sum()
    w = torch.outer(g, g).to(dtype=x.dtype, device=x.device).expand(C, 1, SSIM_WINDOW, SSIM_WINDOW).contiguous()

    def conv(t):
        return torch.nn.functional.conv2d(t, w, padding=r, groups=C)

    X, Y = x.permute(2, 0, 1).unsqueeze(0), y.permute(2, 0, 1).unsqueeze(0)
    mx, my = conv(X), conv(Y)
    sx, sy, sxy = conv(X * X) - mx * mx, conv(Y * Y) - my * my, conv(X * Y) - mx * my
    m = ((2.0 * mx * my + SSIM_C1) * (2.0 * sxy + SSIM_C2)) / ((mx * mx + my * my + SSIM_C1) * (sx + sy + SSIM_C2))
    return m


def _ssim_mean_torch(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """mean SSIM of two (H, W, C) images with torch ops (the CPU path)."""
    return _ssim_map_torch(x, y).mean()


class _DSSIMLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y):
        L = _native.lib()
        H, W, C = x.shape
        want = 1 if ctx.needs_input_grad[0] else 0
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        ws = torch.empty((int(L.gr_ssim_ws_bytes(H, W, C, want)),), dtype=torch.uint8, device=x.device)
        _native.check(L.gr_ssim_fwd(_native.ptr(x), _native.ptr(y), H, W, C, want, _native.ptr(loss), _native.ptr(ws),
                                    ws.numel(), _stream(x)), "gr_ssim_fwd")
        if want:
            ctx.save_for_backward(x, y, ws)  # ws: the three maps of the backward
            ctx.stream = torch.cuda.current_stream(x.device)
        return loss

    @staticmethod
    def backward(ctx, g):
        x, y, ws = ctx.saved_tensors
        L = _native.lib()
        H, W, C = x.shape
        cur = torch.cuda.current_stream(x.device)
        if cur != ctx.stream:
            # a backward driven from another stream than the forward's: ordered after it, and the forward
            # stream's allocator must not reuse the tensors while this stream reads them
            cur.wait_stream(ctx.stream)
            for t in (x, y, ws):
                t.record_stream(cur)
        g = g.contiguous().float()
        gx = torch.empty_like(x)
        _native.check(L.gr_ssim_bwd(_native.ptr(x), _native.ptr(y), H, W, C, _native.ptr(g), _native.ptr(ws), ws.numel(),
                                    _native.ptr(gx), _stream(x)), "gr_ssim_bwd")
        return gx, None


def _ssim_args(name: str, a: torch.Tensor, b: torch.Tensor):
    if a.shape != b.shape:
        raise ValueError(f"{name}: shape mismatch {tuple(a.shape)} vs {tuple(b.shape)}")
    if a.dim() != 3 or not 1 <= a.shape[2] <= 4 or a.numel() == 0:
        raise ValueError(f"{name}: images are (H, W, C) with 1 <= C <= 4, got {tuple(a.shape)}")
    return a.contiguous().float(), b.detach().contiguous().float()


def dssim_loss(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """1 - mean SSIM(pred, target) of two (H, W, C) images, C <= 4; the gradient flows to pred only.
    HIP kernels on the device; the same definition with torch ops on CPU tensors."""
    x, y = _ssim_args("dssim_loss", pred, target)
    if x.device.type != "cuda":
        return 1.0 - _ssim_mean_torch(x, y)
    return _DSSIMLoss.apply(x, y)


def ssim(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """The mean SSIM of two (H, W, C) images as a metric: no gradient, no backward maps written."""
    with torch.no_grad():
        x, y = _ssim_args("ssim", a.detach(), b)
        if x.device.type != "cuda":
            return _ssim_mean_torch(x, y)
        return 1.0 - _DSSIMLoss.apply(x, y)


def psnr(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """-10 log10(mean((a - b)^2)) of two images with values in [0, 1] (peak 1), ``inf`` at zero error; any device."""
    with torch.no_grad():
        if a.shape != b.shape:
            raise ValueError(f"psnr: shape mismatch {tuple(a.shape)} vs {tuple(b.shape)}")
        d = a.detach().float() - b.detach().float()
        return -10.0 * torch.log10(torch.mean(d * d))


def image_metrics(pred: torch.Tensor, target: torch.Tensor) -> dict:
    """The view metrics of held-out evaluation from two (H, W, C) images, composed from existing ops (the reference
    route of ViewShardedFitter.evaluate, and what it uses off the HIP device): 0-d tensors ``l1`` = mean|pred -
    target|, ``mse`` = mean (pred - target)^2, ``psnr`` (``psnr``) and ``ssim`` (``ssim``).  No gradient."""
    with torch.no_grad():
        x, y = _ssim_args("image_metrics", pred.detach(), target)
        d = x - y
        return {"l1": torch.mean(torch.abs(d)), "mse": torch.mean(d * d), "psnr": psnr(x, y), "ssim": ssim(x, y)}


def image_metrics_masked(pred: torch.Tensor, alpha: torch.Tensor, target: torch.Tensor, mask: torch.Tensor) -> dict:
    """The masked view metrics of include/gr_hip.h (gr_eval_view_masked) from a rendered (H, W, 3) image, its (H, W)
    alpha, the target and an (H, W) mask whose values are weights as given (expected in [0, 1]), composed from torch ops
    (the reference route of ViewShardedFitter.evaluate(masks=...), and what it uses off the HIP device).  0-d tensors:
    ``fg_fraction`` = M / HW with M = sum mask, ``fg_l1``, ``fg_mse``, ``fg_ssim`` = the mask-weighted sums of |pred -
    target|, its square and the SSIM map (whole images: the windows are not masked) over 3 M, ``fg_psnr`` = -10 log10
    fg_mse (those four NaN for M = 0), ``sil_l1`` = mean|alpha - mask| and ``sil_iou`` of alpha > 0.5 and mask > 0.5 (1 for
    an empty union).  Element-wise in float32, the sums in float64.  No gradient."""
    with torch.no_grad():
        x, y = _ssim_args("image_metrics_masked", pred.detach(), target)
        H, W = x.shape[:2]
        if x.shape[2] != 3 or tuple(alpha.shape) != (H, W) or tuple(mask.shape) != (H, W):
            raise ValueError(f"image_metrics_masked: an (H, W, 3) image with (H, W) alpha and mask, got {tuple(x.shape)}, "
                             f"{tuple(alpha.shape)}, {tuple(mask.shape)}")
        a, m = alpha.detach().float().to(x.device), mask.detach().float().to(x.device)
        f64 = dict(dtype=torch.float64)
        d = x - y
        w = m[:, :, None]
        M = m.sum(**f64)
        n = 3.0 * M  # (0 / 0 = NaN for an empty mask)
        fg_mse = (w * d * d).sum(**f64) / n
        fa, fm = a > 0.5, m > 0.5
        union = (fa | fm).sum(**f64)
        return {"fg_fraction": M / (H * W), "fg_l1": (w * d.abs()).sum(**f64) / n, "fg_mse": fg_mse,
                "fg_psnr": -10.0 * torch.log10(fg_mse),
                "fg_ssim": (w * _ssim_map_torch(x, y)[0].permute(1, 2, 0)).sum(**f64) / n,
                "sil_l1": (a - m).abs().sum(**f64) / (H * W),
                "sil_iou": torch.where(union > 0, (fa & fm).sum(**f64) / union.clamp(min=1.0), torch.ones_like(union))}


CC_RIDGE = 1e-6  # GR_CC_RIDGE (include/gr_hip.h)


def apply_color_transform(img: torch.Tensor, E: torch.Tensor) -> torch.Tensor:
    """The colour-corrected image of include/gr_hip.h: ``y_k = ((E[k][0] x0 + E[k][1] x1) + E[k][2] x2) + E[k][3]`` of an
    (..., 3) image and a 3 x 4 transform (or its 12 values row-major), element-wise in float32, every product and sum
    rounded on its own in that order (the bits k_eval_view<true> stages); not clamped.  Any device."""
    x = img.float()
    if x.shape[-1] != 3 or E.numel() != 12:
        raise ValueError(f"apply_color_transform: an (..., 3) image and a 3 x 4 transform, got {tuple(img.shape)}, {tuple(E.shape)}")
    e = E.detach().to(device=x.device, dtype=torch.float32).reshape(3, 4)
    x0, x1, x2 = x[..., 0], x[..., 1], x[..., 2]
    return torch.stack([((e[k, 0] * x0 + e[k, 1] * x1) + e[k, 2] * x2) + e[k, 3] for k in range(3)], dim=-1)


def color_correct(pred: torch.Tensor, target: torch.Tensor, ridge: float = CC_RIDGE) -> torch.Tensor:
    """The affine colour transform E (3 x 4 float32 on pred's device, row k the output channel) that best maps the
    (H, W, 3) image ``pred`` onto ``target``: row k minimises ``sum_p (E_k . (x, 1) - t_k)^2 + ridge HW |E_k - e_k|^2``,
    e_k row k of [I | 0] (include/gr_hip.h; the ridge makes images of one colour or one pixel well defined and gives the
    identity when target = pred).  The moments in float64 with torch on the images' device, the 4 x 4 Cholesky solve in
    float64 on the host (22 numbers cross; not every device build has a solver), rounded to float32 once.  No gradient."""
    if not (math.isfinite(ridge) and ridge > 0.0):
        raise ValueError(f"color_correct: ridge must be positive and finite, got {ridge}")
    with torch.no_grad():
        x, y = _ssim_args("color_correct", pred.detach(), target)
        if x.shape[2] != 3:
            raise ValueError(f"color_correct: images are (H, W, 3), got {tuple(x.shape)}")
        hw = x.shape[0] * x.shape[1]
        u = torch.cat([x.double().reshape(hw, 3), torch.ones((hw, 1), dtype=torch.float64, device=x.device)], dim=1)
        A = (u.t() @ u).cpu() / hw + ridge * torch.eye(4, dtype=torch.float64)
        B = (u.t() @ y.double().reshape(hw, 3)).cpu() / hw + ridge * torch.eye(4, 3, dtype=torch.float64)
        sol = torch.cholesky_solve(B, torch.linalg.cholesky(A))  # (4, 3): column k is E_k
        return sol.t().contiguous().float().to(x.device)


def image_metrics_cc(pred: torch.Tensor, target: torch.Tensor, ridge: float = CC_RIDGE) -> dict:
    """image_metrics plus the colour-corrected metrics, composed from existing ops (the reference route of
    ViewShardedFitter.evaluate(color_correct=True), and what it uses off the HIP device): ``cc_transform`` =
    color_correct(pred, target, ridge) and ``cc_l1``, ``cc_mse``, ``cc_psnr``, ``cc_ssim`` = image_metrics of
    apply_color_transform(pred, cc_transform) against target.  No gradient."""
    with torch.no_grad():
        out = image_metrics(pred, target)
        E = color_correct(pred, target, ridge)
        cc = image_metrics(apply_color_transform(pred.detach(), E), target)
        out.update({"cc_" + k: v for k, v in cc.items()})
        out["cc_transform"] = E
        return out


__all__ = ["l1_loss", "dssim_loss", "ssim", "psnr", "image_metrics", "image_metrics_masked", "apply_color_transform",
           "color_correct", "image_metrics_cc"]
