"""The reference of the masked view metrics tests (tests/test_eval_mask_cpu.py, tests/test_eval_mask_gpu.py): a float64
dense restatement of the definition in include/gr_hip.h (gr_eval_view_masked) on tests/ssim_reference.py's SSIM map (the
dense 121-tap window, zero padding, whole images: the windows are not masked), on the float32-rounded inputs.
"""
from __future__ import annotations

import math

import torch

import ssim_reference as ref

KEYS = ("fg_fraction", "fg_l1", "fg_mse", "fg_ssim", "sil_l1", "sil_iou")  # the device row's order


def ssim_map(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """The SSIM map (H, W, C) of two (H, W, C) images in their own dtype (ssim_reference.dssim_dense before its mean)."""
    C = x.shape[2]
    w = ref.window(x.dtype).expand(C, 1, 11, 11).contiguous()

    def conv(t):
        return torch.nn.functional.conv2d(t, w, padding=5, groups=C)

    X, Y = x.permute(2, 0, 1)[None], y.permute(2, 0, 1)[None]
    mx, my = conv(X), conv(Y)
    sx, sy, sxy = conv(X * X) - mx * mx, conv(Y * Y) - my * my, conv(X * Y) - mx * my
    m = ((2 * mx * my + 1e-4) * (2 * sxy + 9e-4)) / ((mx * mx + my * my + 1e-4) * (sx + sy + 9e-4))
    return m[0].permute(1, 2, 0)


def metrics(img, alpha, target, mask) -> dict:
    """The six metrics as Python floats (fg_l1, fg_mse, fg_ssim NaN for an empty mask), fg_psnr, and the two counts of
    the IoU (``inter``, ``union``), from an (H, W, 3) image, its (H, W) alpha, the target and the mask."""
    x, a, t, m = (torch.as_tensor(v).detach().cpu().double() for v in (img, alpha, target, mask))
    H, W = m.shape
    assert x.shape == t.shape == (H, W, 3) and a.shape == (H, W)
    d = x - t
    w = m[:, :, None]
    M = float(m.sum())
    over = (lambda s: float(s) / (3.0 * M)) if M > 0.0 else (lambda s: math.nan)
    fa, fm = a > 0.5, m > 0.5
    inter, union = int((fa & fm).sum()), int((fa | fm).sum())
    mse = over((w * d * d).sum())
    return {"fg_fraction": M / (H * W), "fg_l1": over((w * d.abs()).sum()), "fg_mse": mse,
            "fg_ssim": over((w * ssim_map(x, t)).sum()), "sil_l1": float((a - m).abs().sum()) / (H * W),
            "sil_iou": inter / union if union else 1.0, "inter": inter, "union": union,
            "fg_psnr": (-10.0 * math.log10(mse) if mse > 0.0 else math.inf) if M > 0.0 else math.nan}


def blob_mask(H: int, W: int, soft: bool, seed: int = 0) -> torch.Tensor:
    """An (H, W) float32 mask of one centred elliptic blob covering well over 10 % of the image: binary, or soft with a
    smooth edge in [0, 1]; one pixel of it set to exactly 0.5 (which counts as "not above" for the IoU)."""
    yy = (torch.arange(H, dtype=torch.float32) + 0.5)[:, None] / H - 0.5
    xx = (torch.arange(W, dtype=torch.float32) + 0.5)[None, :] / W - 0.5
    g = torch.Generator().manual_seed(seed)
    r2 = (yy / 0.36) ** 2 + (xx / 0.33) ** 2 + 0.05 * torch.rand((H, W), generator=g)
    m = torch.exp(-2.0 * r2 * r2).clamp(0.0, 1.0) if soft else (r2 < 1.0).float()
    m[H // 2, W // 2] = 0.5
    return m.contiguous()
