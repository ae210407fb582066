"""View-sharded data-parallel multiview fitting on MI355X (one process per GPU, RCCL over xGMI).

The math of one iteration is the reference fit loop's (python/fit_multiview_stub.py:265-325):
activations (:268-275), per-view render + L1 / silhouette / depth losses (:277-305), loss =
sum / V + regularisers (:307-308), backward (:310), Adam (:311), densify/prune every interval with
an Adam reset (:318-325).  What changes is where it runs:

* rank r renders views i = r, r+R, r+2R, ... (R ranks) with the HIP render op and computes
  sum_{i in r} loss_i / V (the regulariser is added on rank 0 only);
* one all_reduce(SUM) of a flat fp32 buffer of every parameter gradient (10 floats per Gaussian
  RGB, 19 with SH degree 1) makes every rank hold the full-loss gradient, so the Adam steps are
  identical on all ranks (up to summation order of the collective);
* densify/prune is decided on rank 0 with the host RNG and broadcast, so parameters stay equal.

Random initialisation and densify jitter are drawn from torch's CPU generator in the same order as
the stub (torch.rand for means, then colours; torch.randn_like for jitter), so a seeded run
reproduces the stub's parameters exactly before the first step.

Run single-GPU:   python 3dgaussian_amd/fit_multiview.py --targets_dir DIR [stub flags]
Run on 8 GPUs:    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 \
                      3dgaussian_amd/fit_multiview.py --targets_dir DIR [stub flags]
"""
from __future__ import annotations

import argparse
import contextlib
import ctypes
import json
import math
import os
import sys
from pathlib import Path
from typing import Callable, Optional

import numpy as np
import torch
import torch.distributed as dist

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import losses  # type: ignore
    import torch_renderer as tr  # type: ignore
    from spatial import _spread3, morton_order  # type: ignore  # noqa: F401
else:
    from . import losses
    from . import torch_renderer as tr
    from .spatial import _spread3, morton_order  # noqa: F401

RenderFn = Callable[..., tuple]


def ctypes_stream(device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
DEVICE_DENSIFY_MIN = 100_000  # Gaussians from which densify/prune runs on the device (C5 scale)
FUSED_LOSS = os.environ.get("GR_FUSED_LOSS", "1") != "0"  # losses.l1_loss for the L1 terms (A/B switch)
# HIP streams the views rotate over (same-box A/B, 20 steps: 4 vs 3 +0.5% at 50 views, +0.8% at the 7 views
# one rank of 8 renders, +2% at 25; 6 or 8 streams lose)
NUM_STREAMS = max(1, int(os.environ.get("GR_STREAMS", "4")))
PREFETCH = max(1, int(os.environ.get("GR_PREFETCH", "3")))  # views prepared ahead of the one rendering
# steps between re-establishing the Morton order of the moving Gaussians (ViewShardedFitter.respatialize;
# 0 = only at construction and after densify/prune).  A re-sort costs ~1.2 ms at 1M Gaussians (codes,
# argsort, 12 permuted tensors); the means move little in 16 Adam steps, so the tile locality holds
# (same-box A/B at C4, 20 steps: 16 vs 4 +1%)
RESORT_EVERY = max(0, int(os.environ.get("GR_RESORT", "16")))
# the fit step without a depth loss renders through the fused path (ViewShardedFitter._views_direct:
# gr_bwd_l1 + per-stream gradient accumulators, no autograd per view); 0 = the autograd path
DIRECT_BACKWARD = os.environ.get("GR_DIRECT", "1") != "0"
# views of one stream whose gradient partials are reduced together (gr_reduce_views): the parameters are
# read and the stream's gradient accumulator read and written once per batch instead of once per view
# (at most REDUCE_BATCH views per batch, a stream's views split into equal batches)
REDUCE_BATCH = max(1, min(16, int(os.environ.get("GR_REDUCE_BATCH", "16"))))
# views in the last batch of each stream (0: near-equal batches only)
REDUCE_TAIL = max(0, min(REDUCE_BATCH, int(os.environ.get("GR_REDUCE_TAIL", "2"))))  # a batch holds <= REDUCE_BATCH
# fused path: gradient assembly through the activations and the Adam update in one HIP pass per parameter
# (gr_fit_param_step) instead of torch's autograd + foreach Adam (0 = torch)
FUSED_STEP = os.environ.get("GR_FUSED_STEP", "1") != "0"
# fused path: views prepared ahead of the one being rendered (on the preparation stream)
PREP_AHEAD = max(1, int(os.environ.get("GR_PREP_AHEAD", "6")))
# views prepared together (gr_fwd_prepare_views_async: the parameters read once for the group)
PREP_GROUP = max(1, min(4, int(os.environ.get("GR_PREP_GROUP", "4"))))
PREP_FIRST = max(1, min(PREP_GROUP, int(os.environ.get("GR_PREP_FIRST", "1"))))
# groups prepared before the step's first render is enqueued: 2 (the first view's group and the next one), or 1
# (only the first view's: the next group is enqueued after the first render)
PREP_INITIAL = max(1, min(2, int(os.environ.get("GR_PREP_INITIAL", "2"))))
# the fused path's reduction in two stages: each view's pair partials gathered into per-Gaussian sums right
# after its backward splat (gr_gather_view: a lean kernel that runs beside the other streams' splats; the view's
# workspaces are released at once), the chain rules of a stream's batch of views from those sums
# (gr_reduce_sums).  0 = the one-pass gr_reduce_views over the batch's kept workspaces.
GATHER = os.environ.get("GR_GATHER", "1") != "0"
# the fused paths' per-view schedule as native host code (gr_fit_views, csrc/gr_fit_exec.cpp: the same streams,
# preparation groups and reduction batches, bit-identical results); 0 = the Python schedule below, 1 = always,
# auto (default) = for views of at most NATIVE_EXEC_MAX_PIXELS, where the per-view GPU work is short enough for the
# host's per-view enqueue time to show (C2, 8 views 512x512: 1.33 -> 1.10 ms per step; at 800x800 the step is
# GPU-bound and the Python schedule is level or 1-2% ahead: profiles/r03_ab_native_exec.txt)
NATIVE_EXEC = os.environ.get("GR_NATIVE_EXEC", "auto")
NATIVE_EXEC_MAX_PIXELS = 512 * 512
# the native executor on this driver's torch streams (1) or on streams of its own (0)
EXEC_STREAMS = os.environ.get("GR_EXEC_STREAMS", "1") != "0"
# priority of the preparation stream (torch's convention: 0 normal, -1 high).  HIP keeps one pool of hardware
# queues per priority, so a high-priority preparation stream also stops sharing a queue with a render stream.
PREP_PRIORITY = int(os.environ.get("GR_PREP_PRIORITY", "0"))
# the fused path's binning (gr_fwd_bin) on a stream of its own with this priority ("" = off: each view bins on
# its render stream inside gr_fwd_render_l1).  The binning kernels are latency-bound; behind the other streams'
# splats they take several times their standalone time while holding CU resources.
BIN_STREAM = os.environ.get("GR_BIN_STREAM", "")
# the fused path at f32 grade (gr_view.no_depth_grad = 2: three-piece splits in both splats, as the default
# precision mode) instead of its two-piece mode: the precision reference of the fit path (bench.py f32_grade_fit)
F32_GRADE = os.environ.get("GR_F32_GRADE", "0") != "0"
# screen tile edge of the fused path's views (gr_view.tile): 32-pixel tiles halve the (Gaussian, tile) pairs of the
# ~3-pixel-sigma C4 scene (7.8 -> 3.7 per Gaussian), so the binning and the per-pair gradient rows and their gather
# (DESIGN.md §5); 16 = the drop-in op's tiles.  The f32-grade reference mode (F32_GRADE) keeps 16.
FIT_TILE = int(os.environ.get("GR_FIT_TILE", "32"))
# How the fused step is enqueued (world size 1; ViewShardedFitter._graph_step): the views are prepared against per-view
# pair capacities (gr_fwd_prepare_views_sized: the counts stay on the device, nothing in the step waits for the host),
# the Adam scalars come from a device table indexed by a device step counter, and a step whose views exceed their
# capacities updates nothing and is redone with larger ones.  Modes (GR_GRAPH):
#   batch       every kernel launched once per batch of up to 8 views (gr_fit_views_batched), one stream: small views
#               fill the GPU (C3 580 -> 765, C2 2,020 -> 2,720 Mpx/s, profiles/r05_batched.txt)
#   batchgraph  that step captured once as a HIP graph and replayed
#   1           the multi-stream step captured and replayed (ROCm runs a captured graph's branches at most two at a
#               time here: slower than eager, profiles/r05_graph_ab.txt)
#   sized/exec  the device-sized multi-stream step enqueued eagerly, Python / native executor (diagnostics)
#   0           the eager multi-stream step, host-sized
#   auto        (default) batch for views of at most GRAPH_AUTO_PIXELS, else 0: at 800x800 the per-view launches already
#               fill the GPU and the eager step's stream overlap wins (C4 1,557 eager vs 1,446 batched)
GRAPH_MODE = os.environ.get("GR_GRAPH", "auto")
GRAPH_AUTO_PIXELS = 512 * 512
# multi-GPU: the r = V mod R views left over by the even split are cut into bands of tile rows (gr_view.row0 / rows),
# the ranks split into r groups, one per leftover view, each group cutting its view into as many bands as it has ranks:
# every rank renders V // R views and ONE band (50 views on 8 ranks: 6 views and a quarter view each instead of 7 on
# two ranks; round 5 gave every rank a band of every leftover view, two eighths, each paying a band's fixed cost); the
# fused path without a depth term only (a depth term needs the whole image's depth maximum).  0 = whole views round-robin.
BAND_SPLIT = os.environ.get("GR_BAND_SPLIT", "1") != "0"
# a band costs about this fraction of a whole view beyond its share of the view's pairs (its preparation, binning
# launches, gather and chain rule run over every Gaussian: ~90 of ~560 us single-stream at C4, tools/band_probe.py;
# more in the overlapped step): the split is used when the most loaded rank's band (this plus its largest share of the
# pairs) is below a whole view.  Measured per rank (profiles/r06_rank_share.txt): C4 at 8 ranks, quarter-view bands
# (29% of the pairs): 3.25 -> 3.02-3.10 ms for every rank; at 4 ranks, half-view bands: 5.82 -> 6.13-6.19, so 0.5 keeps
# whole views there
BAND_OVERHEAD = float(os.environ.get("GR_BAND_OVERHEAD", "0.5"))
GRAPH_MARGIN = float(os.environ.get("GR_GRAPH_MARGIN", "1.25"))  # capacity over the counts seen (+ 4096 pairs)


# ------------------------------------------------------------------------------------------------
# Parameters (fit_multiview_stub.py:114-137) — CPU RNG, then moved to the device.
# ------------------------------------------------------------------------------------------------
def build_params(n: int, device: torch.device, use_sh: bool, sh_degree: int = 1) -> dict:
    """sh_degree 3 (extension, config C3): (N,16,3) coefficients, the degree-1 init of the stub plus
    zero degree-2/3 terms."""
    means = (torch.rand((n, 3)) - 0.5) * 1.2
    scales_raw = torch.full((n, 3), -2.2)
    opacities_raw = torch.full((n,), -2.2)
    params = {"means": means, "scales_raw": scales_raw, "opacities_raw": opacities_raw}
    if use_sh:
        sh = torch.zeros((n, 16 if sh_degree == 3 else 4, 3))
        sh[:, 0, :] = 0.1 * torch.rand((n, 3))
        params["sh_raw"] = sh
    else:
        params["colors_raw"] = 0.1 * torch.rand((n, 3))
    return {k: torch.nn.Parameter(v.to(device)) for k, v in params.items()}


def activations(params: dict):
    """fit_multiview_stub.py:268-275.  Leaf parameters used as they are (means, SH coefficients) pass
    through a view, so the per-view gradients that arrive from the render streams meet in a node made on
    this (the main) stream rather than in the leaf's accumulator."""
    means = params["means"].view(params["means"].shape)
    scales = torch.nn.functional.softplus(params["scales_raw"]) + 1e-3
    opacities = torch.sigmoid(params["opacities_raw"])
    colors = params["sh_raw"].view(params["sh_raw"].shape) if "sh_raw" in params else torch.sigmoid(params["colors_raw"])
    return means, scales, colors, opacities


def activations_native(params: dict, reg=None, ws=None):
    """activations() in one HIP launch (gr_fit_activations: the same float formulas as torch's softplus and
    sigmoid), for the fused step, which needs no autograd graph; with reg = (reg_opacity, reg_scale) also the
    regulariser reg_opacity * mean(opacities) + reg_scale * mean(scales) (fit_multiview_stub.py:307-308) as a 0-d
    device tensor, summed in the same launch (ws: a zeroed uint8 tensor of gr_fit_activations_ws_bytes).
    Returns (means, scales, colors, opacities, reg or None)."""
    nat = tr._native
    L = nat.lib()
    means = params["means"].detach()
    sr, orw = params["scales_raw"].detach().contiguous(), params["opacities_raw"].detach().contiguous()
    cr = params["colors_raw"].detach().contiguous() if "colors_raw" in params else None
    n = int(means.shape[0])
    scales, opacities = torch.empty_like(sr), torch.empty_like(orw)
    colors = torch.empty_like(cr) if cr is not None else params["sh_raw"].detach()
    out = torch.empty((), dtype=torch.float32, device=means.device) if reg is not None and n > 0 else None
    nat.check(L.gr_fit_activations(n, nat.ptr(sr), nat.ptr(orw), nat.ptr(cr) if cr is not None else None,
                                   int(cr.numel()) if cr is not None else 0, nat.ptr(scales), nat.ptr(opacities),
                                   nat.ptr(colors) if cr is not None else None,
                                   ctypes.c_float(reg[1] if reg else 0.0), ctypes.c_float(reg[0] if reg else 0.0),
                                   nat.ptr(out) if out is not None else None,
                                   ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0,
                                   ctypes_stream(means.device)), "gr_fit_activations")
    return means, scales, colors, opacities, out


def prune_by_contribution(peak: torch.Tensor, threshold: float, min_keep: int = 64) -> torch.Tensor:
    """The keep mask of contribution-based pruning: ``peak > threshold`` (ViewShardedFitter.contribution_state: each
    Gaussian's largest blend weight w / (1 + W) over the training views' pixels; removing one with peak <= t moves no
    training pixel by more than t / (1 - t)); if fewer than ``min_keep`` survive, the ``min_keep`` largest ``peak``
    instead, ties to the lower index (the opacity rule's floor of 64)."""
    keep = peak > threshold
    if int(keep.sum()) < min_keep:
        top = torch.sort(peak, descending=True, stable=True).indices[:min(min_keep, peak.shape[0])]
        keep = torch.zeros_like(keep, dtype=torch.bool)
        keep[top] = True
    return keep


def _keep_mask(keep: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    """A caller's keep mask for the densify rules: (N,) bool on the rule's device."""
    if keep.dtype != torch.bool or tuple(keep.shape) != tuple(like.shape):
        raise ValueError(f"keep: expected a bool mask of shape {tuple(like.shape)}, got {keep.dtype} {tuple(keep.shape)}")
    return keep.to(like.device)


def densify_and_prune(params: dict, max_gaussians: int, densify_ratio: float, prune_opacity: float,
                      keep: Optional[torch.Tensor] = None) -> dict:
    """fit_multiview_stub.py:140-197, evaluated on the host (CPU RNG for the jitter) so that every
    rank that calls it with the same RNG state gets identical parameters.  ``keep`` ((N,) bool, e.g.
    prune_by_contribution's): the rows that survive, in place of the opacity rule and its floor of 64."""
    with torch.no_grad():
        cpu = {k: v.detach().cpu() for k, v in params.items()}
        means, scales_raw, op_raw = cpu["means"], cpu["scales_raw"], cpu["opacities_raw"]
        op = torch.sigmoid(op_raw)
        scales = torch.nn.functional.softplus(scales_raw) + 1e-3
        if keep is not None:
            keep = _keep_mask(keep, op)
        else:
            keep = op > prune_opacity
            if int(keep.sum()) < 64:
                top_keep = torch.topk(op, k=min(64, op.shape[0]), largest=True).indices
                keep = torch.zeros_like(keep, dtype=torch.bool)
                keep[top_keep] = True
        means, scales_raw, op_raw, scales = means[keep], scales_raw[keep], op_raw[keep], scales[keep]
        op = torch.sigmoid(op_raw)
        n = means.shape[0]
        room = max(0, max_gaussians - n)
        add_n = min(room, max(0, int(n * densify_ratio)))
        if add_n > 0 and n > 0:
            idx = torch.topk(op, k=min(n, add_n), largest=True).indices
            jitter = 0.25 * scales[idx] * torch.randn_like(means[idx])
            means = torch.cat([means, means[idx] + jitter], dim=0)
            scales_raw = torch.cat([scales_raw, scales_raw[idx]], dim=0)
            op_raw = torch.cat([op_raw, op_raw[idx] - 0.1], dim=0)
        out = {"means": means, "scales_raw": scales_raw, "opacities_raw": op_raw}
        key = "sh_raw" if "sh_raw" in cpu else "colors_raw"
        col = cpu[key][keep]
        if add_n > 0 and col.shape[0] > 0:
            base_n = col.shape[0]
            idx = torch.topk(torch.sigmoid(op_raw[:base_n]), k=min(base_n, add_n), largest=True).indices
            col = torch.cat([col, col[idx]], dim=0)
        out[key] = col
    device = params["means"].device
    return {k: torch.nn.Parameter(v.to(device)) for k, v in out.items()}


def densify_and_prune_device(params: dict, max_gaussians: int, densify_ratio: float, prune_opacity: float,
                             generator: Optional[torch.Generator] = None, noise: Optional[torch.Tensor] = None,
                             keep: Optional[torch.Tensor] = None) -> dict:
    """The same rule as densify_and_prune (fit_multiview_stub.py:140-197) evaluated on the device, for
    fits at scale (config C5: millions of Gaussians), with the jitter drawn from a device generator:
    no host round trip of the parameters.  Same keep / top-k / jitter / -0.1 opacity / colour
    duplication; only the random stream differs from the stub's CPU one.  ``noise`` (>= added rows x 3,
    standard normal) replaces the generator's draw: with the stub's own draw the result is the host
    rule's (tests/test_densify.py).  ``keep``: as densify_and_prune's."""
    with torch.no_grad():
        means, scales_raw, op_raw = params["means"].detach(), params["scales_raw"].detach(), params["opacities_raw"].detach()
        key = "sh_raw" if "sh_raw" in params else "colors_raw"
        col = params[key].detach()
        op = torch.sigmoid(op_raw)
        if keep is not None:
            keep = _keep_mask(keep, op)
        else:
            keep = op > prune_opacity
            if int(keep.sum()) < 64:
                top_keep = torch.topk(op, k=min(64, op.shape[0]), largest=True).indices
                keep = torch.zeros_like(keep, dtype=torch.bool)
                keep[top_keep] = True
        means, scales_raw, op_raw, col = means[keep], scales_raw[keep], op_raw[keep], col[keep]
        n = means.shape[0]
        room = max(0, max_gaussians - n)
        add_n = min(room, max(0, int(n * densify_ratio)))
        if add_n > 0 and n > 0:
            idx = torch.topk(torch.sigmoid(op_raw), k=min(n, add_n), largest=True).indices
            scales = torch.nn.functional.softplus(scales_raw[idx]) + 1e-3
            if noise is not None:
                z = noise[:idx.shape[0]].to(device=means.device, dtype=means.dtype)
            else:
                z = torch.randn(means[idx].shape, generator=generator, device=means.device, dtype=means.dtype)
            jitter = 0.25 * scales * z
            means = torch.cat([means, means[idx] + jitter], dim=0)
            scales_raw = torch.cat([scales_raw, scales_raw[idx]], dim=0)
            col = torch.cat([col, col[idx]], dim=0)
            op_raw = torch.cat([op_raw, op_raw[idx] - 0.1], dim=0)
        out = {"means": means, "scales_raw": scales_raw, "opacities_raw": op_raw, key: col}
    return {k: torch.nn.Parameter(v.contiguous()) for k, v in out.items()}


def densify_by_gradient(params: dict, gsum: torch.Tensor, seen: torch.Tensor, grad_threshold: float, split_scale: float,
                        max_gaussians: int, prune_opacity: float, generator: Optional[torch.Generator] = None,
                        noise: Optional[torch.Tensor] = None, keep: Optional[torch.Tensor] = None) -> dict:
    """Adaptive density control (an extension: the stub's rule, densify_and_prune, duplicates the most opaque Gaussians)
    from the fit's density statistics (ViewShardedFitter.density_state: per Gaussian the sum over the views that saw it
    of the view loss's gradient norm w.r.t. its NDC position, and the number of those views), on the tensors' device:
      1. prune as densify_and_prune (sigmoid(opacities_raw) > prune_opacity, else the 64 most opaque; or the rows of
         ``keep`` when given);
      2. avg = gsum / max(seen, 1); candidates: kept rows with seen > 0 and avg >= grad_threshold, at most
         max_gaussians - kept of them (each adds one row net), the largest avg first, ties to the lower index;
      3. with s = softplus(scales_raw) + 1e-3 and smax its larger screen-plane component (columns 0, 1, the two the
         renderer reads): smax <= split_scale clones the row; smax > split_scale splits it: the parent leaves, two
         children at m + s * z (z standard normal, 3 columns) with scales s / 1.6, the parent's colour and opacity.
    Output rows: the survivors in order, the clones in parent order, then each split parent's two children in parent
    order (``noise[2k]``, ``noise[2k + 1]`` for the k-th split; else drawn from ``generator``): deterministic given
    ``noise``."""
    with torch.no_grad():
        means, scales_raw, op_raw = params["means"].detach(), params["scales_raw"].detach(), params["opacities_raw"].detach()
        key = "sh_raw" if "sh_raw" in params else "colors_raw"
        col = params[key].detach()
        dev = means.device
        op = torch.sigmoid(op_raw)
        if keep is not None:
            keep = _keep_mask(keep, op)
        else:
            keep = op > prune_opacity
            if int(keep.sum()) < 64:
                top_keep = torch.topk(op, k=min(64, op.shape[0]), largest=True).indices
                keep = torch.zeros_like(keep, dtype=torch.bool)
                keep[top_keep] = True
        gsum, seen = gsum.to(dev), seen.to(dev)
        avg = gsum / seen.clamp_min(1.0)
        idx = torch.nonzero(keep & (seen > 0) & (avg >= grad_threshold)).flatten()
        room = max(0, max_gaussians - int(keep.sum()))
        if idx.numel() > room:  # a stable sort: equal averages keep their index order
            first = torch.sort(avg[idx], descending=True, stable=True).indices[:room]
            idx = torch.sort(idx[first]).values
        return _clone_split(means, scales_raw, op_raw, key, col, keep, idx, split_scale, generator, noise)


def _clone_split(means, scales_raw, op_raw, key: str, col, keep, idx, split_scale: float, generator, noise) -> dict:
    """Step 3 of densify_by_gradient, shared with densify_by_error: of the candidate rows ``idx`` (ascending, all kept)
    clone the small and split the large, and assemble the output rows in the documented order."""
    dev = means.device
    s = torch.nn.functional.softplus(scales_raw[idx]) + 1e-3
    split = s[:, :2].max(dim=1).values > split_scale
    clones, parents, sp = idx[~split], idx[split], s[split]
    survive = keep.clone()
    survive[parents] = False
    k2 = 2 * int(parents.numel())
    if noise is not None:
        z = noise[:k2].to(device=dev, dtype=means.dtype)
    else:
        z = torch.randn((k2, 3), generator=generator, device=dev, dtype=means.dtype)
    two = parents.repeat_interleave(2)
    child_means = means[two] + sp.repeat_interleave(2, dim=0) * z
    # softplus^-1 of s / 1.6 (torch's softplus is the identity above its threshold of 20)
    a = (sp / 1.6 - 1e-3).clamp_min(1e-6)
    child_raw = torch.where(a > 20.0, a, torch.log(torch.expm1(a))).repeat_interleave(2, dim=0)
    out = {"means": torch.cat([means[survive], means[clones], child_means]),
           "scales_raw": torch.cat([scales_raw[survive], scales_raw[clones], child_raw]),
           "opacities_raw": torch.cat([op_raw[survive], op_raw[clones], op_raw[two]]),
           key: torch.cat([col[survive], col[clones], col[two]])}
    return {k: torch.nn.Parameter(v.contiguous()) for k, v in out.items()}


def densify_by_error(params: dict, err: torch.Tensor, threshold: float, split_scale: float, max_gaussians: int,
                     prune_opacity: float, max_new: Optional[int] = None, generator: Optional[torch.Generator] = None,
                     noise: Optional[torch.Tensor] = None, keep: Optional[torch.Tensor] = None,
                     report: Optional[dict] = None) -> dict:
    """Error-driven density control (an extension) from each Gaussian's blend-weighted pixel error
    (ViewShardedFitter.error_state: the largest, over the training views, of its share sum_p b_i(p) e(p) of the view's
    L1 error, b = w / (1 + W) the blend weight), on the tensors' device:
      1. prune as densify_and_prune (or the rows of ``keep`` when given);
      2. candidates: kept rows with err > threshold, at most min(max_gaussians - kept, max_new) of them (each adds one
         row net; max_new None: no second cap), the largest err first, ties to the lower index;
      3. densify_by_gradient's clone / split step on them (_clone_split): the same output row order and ``noise``
         contract.
    ``report`` (a dict) receives the numbers of ``clones`` and ``splits`` made."""
    with torch.no_grad():
        means, scales_raw, op_raw = params["means"].detach(), params["scales_raw"].detach(), params["opacities_raw"].detach()
        key = "sh_raw" if "sh_raw" in params else "colors_raw"
        col = params[key].detach()
        op = torch.sigmoid(op_raw)
        if keep is not None:
            keep = _keep_mask(keep, op)
        else:
            keep = op > prune_opacity
            if int(keep.sum()) < 64:
                top_keep = torch.topk(op, k=min(64, op.shape[0]), largest=True).indices
                keep = torch.zeros_like(keep, dtype=torch.bool)
                keep[top_keep] = True
        err = err.to(means.device)
        if tuple(err.shape) != tuple(op.shape):
            raise ValueError(f"err: expected shape {tuple(op.shape)}, got {tuple(err.shape)}")
        idx = torch.nonzero(keep & (err > threshold)).flatten()
        room = max(0, max_gaussians - int(keep.sum()))
        if max_new is not None:
            room = min(room, max(0, int(max_new)))
        if idx.numel() > room:  # a stable sort: equal errors keep their index order
            first = torch.sort(err[idx], descending=True, stable=True).indices[:room]
            idx = torch.sort(idx[first]).values
        if report is not None:
            s = torch.nn.functional.softplus(scales_raw[idx]) + 1e-3
            report["splits"] = int((s[:, :2].max(dim=1).values > split_scale).sum())
            report["clones"] = int(idx.numel()) - report["splits"]
        return _clone_split(means, scales_raw, op_raw, key, col, keep, idx, split_scale, generator, noise)


def spatial_order(params: dict) -> dict:
    """The same Gaussians, permuted into morton_order (a layout choice of the trainer: the rendered
    images and the loss do not depend on the order of the Gaussians beyond float summation order)."""
    if params["means"].shape[0] < 2:
        return params
    perm = morton_order(params["means"])
    return {k: torch.nn.Parameter(v.detach()[perm].contiguous()) for k, v in params.items()}


def _fit_images(name: str, imgs: Optional[list], shape: tuple, device) -> tuple:
    """The fused fit path reads the targets / masks / depths through raw device pointers (gr_fwd_render_l1,
    gr_bwd_fit): each must be exactly ``shape``, float32, contiguous, on the parameters' device.  Returns
    (images, ok): images normalised to that (a copy only where the dtype, layout or device differ), ok =
    False when a shape differs (the fit then takes the autograd path, which broadcasts or raises as torch
    does for the stub's expressions)."""
    if imgs is None:
        return None, True
    if any(tuple(t.shape) != shape for t in imgs):
        return list(imgs), False
    return [torch.as_tensor(t).to(device=device, dtype=torch.float32).contiguous() for t in imgs], True


def _fit_weights(weights: Optional[list], count: int, shape: tuple, device) -> tuple:
    """The per-pixel loss weights of a fit (ViewShardedFitter(weights=...)), checked once: one map per training view,
    exactly ``shape`` = (H, W), a real floating-point dtype, finite and >= 0 after conversion to float32.  Returns
    (maps, ok) as _fit_images does (float32, contiguous, on ``device``)."""
    if weights is None:
        return None, True
    weights = list(weights)
    if len(weights) != count:
        raise ValueError(f"weights: expected one map per training view ({count}), got {len(weights)}")
    maps = []
    for i, w in enumerate(weights):
        w = torch.as_tensor(w)
        if tuple(w.shape) != tuple(shape):
            raise ValueError(f"weights[{i}]: expected shape {tuple(shape)} (height, width), got {tuple(w.shape)}")
        if not w.is_floating_point():
            raise ValueError(f"weights[{i}]: expected a floating-point dtype (converted to float32), got {w.dtype}")
        w = w.detach().to(dtype=torch.float32)
        if not bool(torch.isfinite(w).all()):
            raise ValueError(f"weights[{i}]: every weight must be finite (a NaN or an infinity after conversion to float32)")
        if bool((w < 0).any()):
            raise ValueError(f"weights[{i}]: every weight must be >= 0, got a minimum of {float(w.min()):g}")
        maps.append(w)
    return _fit_images("weights", maps, tuple(shape), device)


def _batch_sizes(ns: int, nviews: int, tail: Optional[int] = None) -> list:
    """Per stream (views j = k, k + ns, ...): its views' reduction batches, near-equal and at most REDUCE_BATCH, in
    the order they fill; a short last batch of REDUCE_TAIL views (the reductions left when the renders end run alone).
    The native executor's schedule() is the same rule."""
    sizes = []
    for k in range(ns):
        p = len(range(k, nviews, ns))
        rt = REDUCE_TAIL if tail is None else tail
        t = min(rt, REDUCE_BATCH) if 0 < rt < p else 0  # (gr_fit_views: tail <= batch)
        nb = max(1, -(-(p - t) // REDUCE_BATCH))
        sizes.append([(p - t) // nb + (1 if b < (p - t) % nb else 0) for b in range(nb)] + ([t] if t else []))
    return sizes


def _int_hist(idx: torch.Tensor, wts: torch.Tensor, nb: int) -> torch.Tensor:
    """Sum of the int64 weights per bin 0..nb-1 (indices in range): sorted indices, prefix sums, bin ends."""
    srt, order = torch.sort(idx)
    cw = torch.cumsum(wts[order], 0)
    ends = torch.searchsorted(srt, torch.arange(nb, device=idx.device, dtype=srt.dtype), right=True)
    upto = torch.where(ends > 0, cw[(ends - 1).clamp_min(0)], torch.zeros_like(ends))
    return torch.diff(upto, prepend=torch.zeros(1, dtype=upto.dtype, device=upto.device))


def _min_max_cuts(w, g: int) -> list:
    """Boundaries 0 = c_0 < c_1 < ... < c_g = len(w) of g non-empty contiguous runs of `w` whose largest sum is
    the smallest possible (dynamic programming over the cut positions; ties to the earliest cut)."""
    n = len(w)
    c = np.concatenate([[0.0], np.cumsum(np.asarray(w, np.float64))])
    best = np.full((g + 1, n + 1), np.inf)
    arg = np.zeros((g + 1, n + 1), np.int64)
    best[0, 0] = 0.0
    for k in range(1, g + 1):
        for j in range(k, n - (g - k) + 1):
            for i in range(k - 1, j):
                v = max(best[k - 1, i], c[j] - c[i])
                if v < best[k, j]:
                    best[k, j], arg[k, j] = v, i
    cuts = [n]
    for k in range(g, 0, -1):
        cuts.append(int(arg[k, cuts[-1]]))
    return cuts[::-1]


def bucketed_all_reduce(buckets: list, assemble: Callable[[int], None], finish: Callable[[int], None], group=None) -> None:
    """The step's one real exchange (SUM over ranks) in buckets, one per parameter tensor (plus the loss in
    the last): bucket b is assembled (``assemble(b)``, on the current stream) and its all-reduce issued
    asynchronously at once, so RCCL moves bucket b over xGMI while bucket b + 1 is assembled; then each
    bucket's update (``finish(b)``) waits for its own all-reduce only.  Summation order per element is the
    collective's, as for one flat buffer."""
    works = []
    for b in range(len(buckets)):
        assemble(b)
        works.append(dist.all_reduce(buckets[b], op=dist.ReduceOp.SUM, group=group, async_op=True))
    for b, w in enumerate(works):
        w.wait()
        finish(b)


# The row of the masked view metrics (gr_eval_view_masked; fg_psnr is formed from fg_mse on the host)
MASK_KEYS = ("fg_fraction", "fg_l1", "fg_mse", "fg_ssim", "sil_l1", "sil_iou")


def hip_render(means, scales, colors, opacities, cam, width, height, background, prepared=None, depth_grad=True):
    return tr.render_gaussians_torch(means, scales, colors, opacities, cam, width=width, height=height,
                                     background=background, max_gaussians=max(10000, int(means.shape[0])), return_aux=True,
                                     prepared=prepared, depth_grad=depth_grad)


def pose_view(xi: torch.Tensor, view0: torch.Tensor) -> torch.Tensor:
    """The view matrix of a camera whose pose is refined: ``E(xi) @ view0`` with ``xi = (omega, tau)`` (6 values),
    ``E = [[R(omega), tau], [0, 1]]`` and R the rotation-vector exponential (Rodrigues), a left perturbation in the
    camera's frame.  Plain differentiable torch; leading batch dimensions pass through (xi (..., 6), view0 (..., 4, 4)).
    ``E(0) = I`` exactly (so ``pose_view(0, V) == V`` bit for bit), the Jacobian at 0 is the six generators of se(3),
    and view0's last row is kept."""
    xi = xi.to(view0.dtype)
    w, tau = xi[..., :3], xi[..., 3:6]
    t2 = (w * w).sum(-1)
    small = t2 < 1e-12
    t2s = torch.where(small, torch.ones_like(t2), t2)  # (no sqrt at 0: its derivative is not finite)
    th = torch.sqrt(t2s)
    a = torch.where(small, 1.0 - t2 / 6.0, torch.sin(th) / th)
    b = torch.where(small, 0.5 - t2 / 24.0, 2.0 * torch.sin(0.5 * th) ** 2 / t2s)
    z = torch.zeros_like(t2)
    K = torch.stack([torch.stack([z, -w[..., 2], w[..., 1]], -1), torch.stack([w[..., 2], z, -w[..., 0]], -1),
                     torch.stack([-w[..., 1], w[..., 0], z], -1)], -2)
    eye = torch.eye(3, dtype=view0.dtype, device=view0.device)
    KK = w[..., :, None] * w[..., None, :] - t2[..., None, None] * eye  # K @ K
    E = torch.cat([eye + a[..., None, None] * K + b[..., None, None] * KK, tau[..., None]], dim=-1)
    # the product term by term (element-wise operations only: the same bits for one view or a batch, on every rank)
    top = (E[..., :, 0:1] * view0[..., 0:1, :] + E[..., :, 1:2] * view0[..., 1:2, :] + E[..., :, 2:3] * view0[..., 2:3, :]
           + E[..., :, 3:4] * view0[..., 3:4, :])
    return torch.cat([top, view0[..., 3:4, :]], dim=-2)


class _EagerReplay:
    """GR_GRAPH=sized: replay() enqueues the device-sized step again instead of launching a captured graph."""

    def __init__(self, body, gs):
        self.body, self.gs = body, gs

    def replay(self):
        self.gs.loss = self.body()


class _GraphState:
    """The captured fused step (ViewShardedFitter._graph_build) and its device-side sizing state."""

    def __init__(self):
        self.graph = None
        self.key = None
        self.sched = None
        self.sched_len = 0
        self.sched_key = None
        self.overflows = 0  # steps redone with larger capacities (tests, bench)
        self.builds = 0  # captures
        self.inflight = []


class ViewShardedFitter:
    """One fit iteration = render own views, backward, one gradient all-reduce, Adam.

    On the fused path every parameter's ``.grad`` after ``step()`` is a tensor the fitter keeps and overwrites in
    place on the next step (no allocation per step): copy it to keep a step's gradient."""

    def __init__(self, params: dict, cams: list, targets: list, width: int, height: int, lr: float = 0.02,
                 masks: Optional[list] = None, depths: Optional[list] = None, silhouette_weight: float = 0.2,
                 depth_weight: float = 0.05, reg_opacity: float = 1e-3, reg_scale: float = 1e-3,
                 render_fn: RenderFn = hip_render, group=None, reorder: bool = True, dssim_weight: float = 0.0,
                 dssim_fused: bool = False, density_stats: bool = False, refine_cameras: bool = False,
                 camera_lr: float = 1e-3, camera_fixed: tuple = (0,), exposure: bool = False, exposure_lr: float = 1e-3,
                 exposure_fixed: tuple = (0,), exposure_fused: bool = False, weights: Optional[list] = None):
        # dssim_weight l > 0: a view's photometric term is (1 - l) mean|pred - tgt| + l dssim(pred, tgt)
        # (losses.dssim_loss) on the per-view autograd path; 0 (default): the L1 fit, every path as it was
        # dssim_fused (with l > 0, the HIP render op): the fused path's D-SSIM form (_views_scheduled or the native
        # executor: gr_bwd_fit_ssim_gather per view, no autograd and no gradient image) instead of the autograd path
        # density_stats: accumulate every Gaussian's screen-space positional gradient over the views that see it
        # (density_state; what densify_and_prune(mode="gradient") reads): on the HIP device from the fused paths only
        # (gr_density_stats beside every gr_reduce_sums), on other devices from cpu_renderer's position gradients
        # refine_cameras: the views' poses are fitted with the Gaussians (pose_view: a 6-vector per view, an Adam of its
        # own at camera_lr; the views of camera_fixed keep their poses, which pins the scene's gauge): on the HIP device's
        # fused paths from gr_camera_grads_sums beside every gr_reduce_sums, elsewhere through autograd
        # exposure: per-view exposure compensation, a 3 x 4 colour transform E per training view (from [I | 0]) fitted
        # with the scene by an Adam of its own at exposure_lr: the photometric term (L1 and D-SSIM alike) compares
        # E (pred, 1) with the target (the views of exposure_fixed keep theirs, which pins the overall brightness
        # gauge), through autograd in view_loss on host tensors.  On the HIP device exposure alone raises rather than
        # leave the fused path; exposure_fused opts into the fused path's exposure form (_views_scheduled's "exposure":
        # gr_bwd_fit_exposure_gather per view reads E from the device and writes d loss / d E, the Python schedule with
        # the fused parameter step only, no D-SSIM term); on host tensors it changes nothing.  evaluate() renders without E
        # weights: per-pixel loss weights, one (H, W) map per training view, finite and >= 0: every L1 term of pixel p
        # (photometric, silhouette, depth) counts weights[i][p] times, the means keep their denominators 3 HW / HW (ones
        # are the fit without weights bit for bit, 0 a pixel the fit does not see); the depth maximum and its arg-max
        # count stay unweighted.  On host tensors element-wise in view_loss (with or without exposure); on the HIP device
        # the fused path's weighted form (_views_scheduled's "weighted": gr_bwd_fit_weighted_gather per view, the Python
        # schedule with the fused parameter step).  No D-SSIM term; evaluate(), contribution_state() and error_state()
        # do not see the weights
        # reorder: keep the Gaussians in spatial (Morton) order, re-established after every
        # densify/prune (spatial_order); off only to compare with an unpermuted run
        # perm: self.params[k][i] = canonical[k][perm[i]], the canonical order being the stub's (the
        # order densify_and_prune and gaussians_fitted.npz see: top-k ties and jitter draws follow it)
        self.reorder = reorder
        self.perm = None
        self.group = group
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            # data parallelism needs identical replicas: rank 0's initial parameters win (the Morton
            # permutation below is then computed from identical means on every rank)
            src = dist.get_global_rank(group, 0) if group is not None else 0
            for k in sorted(params):
                dist.broadcast(params[k].data, src, group=group)
        if reorder and params["means"].shape[0] >= 2:
            self.perm = morton_order(params["means"])
            params = {k: torch.nn.Parameter(v.detach()[self.perm].contiguous()) for k, v in params.items()}
        self.params = params
        dev = params["means"].device
        targets, ok_t = _fit_images("targets", targets, (height, width, 3), dev)
        masks, ok_m = _fit_images("masks", masks, (height, width), dev)
        depths, ok_d = _fit_images("depths", depths, (height, width), dev)
        weights, ok_w = _fit_weights(weights, len(targets), (height, width), dev)
        self._images_ok = ok_t and ok_m and ok_d and ok_w  # the fused path's exact-shape precondition
        self.cams, self.targets, self.masks, self.depths = cams, targets, masks, depths
        self.weights = weights
        self.width, self.height, self.lr = width, height, lr
        self.w_sil, self.w_depth = silhouette_weight, depth_weight
        if not 0.0 <= dssim_weight <= 1.0:
            raise ValueError(f"dssim_weight must be in [0, 1], got {dssim_weight}")
        self.w_dssim = float(dssim_weight)
        self.dssim_fused = bool(dssim_fused)
        self.reg_opacity, self.reg_scale = reg_opacity, reg_scale
        self.render_fn = render_fn
        self.group = group
        self.distributed = dist.is_available() and dist.is_initialized()
        self.rank = dist.get_rank(group) if self.distributed else 0
        self.world = dist.get_world_size(group) if self.distributed else 1
        self._rr_views = list(range(self.rank, len(targets), self.world))
        self._bands = {}  # virtual view id (>= V) -> (view, first tile row, tile rows) of this rank's bands
        self.opt = torch.optim.Adam(list(self.params.values()), lr=lr)
        self.densify_seed = 1234
        self.steps_done = 0
        # ---- what a fitter keeps between calls, made on first use (None / empty until then) ----
        self._bg = None  # the background colour as one device tensor (_background)
        self._side = []  # the render streams besides the caller's (_streams: grows, never shrinks)
        self._prep = None  # the preparation stream (_streams)
        self._bin = None  # the L1 form's binning stream (GR_BIN_STREAM)
        self._gv = {}  # every cached gr_view, by (kind, ...) (_gr_view); a camera update drops it (_drop_views)
        self._native_targets = None  # (key, GrFitTarget array) of the executor's last fit call; dropped with _gv
        self._acc_kept = {}  # "direct" / "native" -> (shapes, stream accumulator sets, their pointer array) (_acc_sets)
        self._acc_parts = None  # the accumulator sets this step's views wrote, for the parameter update to sum
        self._acc = None  # their sum in stream order while the autograd update reads it
        self._exec_streams = None  # the render streams' handles an executor call reads (_exec_config)
        self._native_keep = None  # the activations the executor's / batched step's streams still read
        self._eval_keep = None  # the same for evaluate() and contribution_state()
        self._pins = None  # pinned (views, 3) int64 rows the preparations write their plans to (_plan_pins)
        self._grad_keep = {}  # parameter name -> its .grad tensor on the fused path, overwritten every step
        self._act_ws = None  # activations_native's workspace (_act_ws_for)
        self._gs = None  # the _GraphState of the device-sized / captured step (_graph_build)
        self._dgen = None  # the device generator of densify_and_prune's device rules
        self._cuts_cache = {}  # band cuts by (view, bands, tile, Gaussians, re-sort epoch) (_band_cuts)
        self._rows_cache = {}  # estimated pairs per tile row by (view, tile, Gaussians, re-sort epoch)
        self._cam_ws = {}  # render stream -> its gr_camera_grads_sums workspace (_camera_ws)
        self._cam_pin = None  # pinned host copy of the step's camera-gradient rows (_camera_step_fused)
        # (density_report / contribution_report / error_report exist only once densify_and_prune has filled them)
        self.density_stats = bool(density_stats)
        self._stats = []  # one (n, 2) buffer per render stream: [sum of gradient norms, seeing views]
        if self.density_stats and dev.type == "cuda":
            self._density_check(dev)
        self.refine_cameras = bool(refine_cameras)
        if self.refine_cameras:
            V = len(cams)
            self.camera_lr = float(camera_lr)
            self.camera_fixed = tuple(sorted({int(i) for i in camera_fixed}))
            if any(not 0 <= i < V for i in self.camera_fixed):
                raise ValueError(f"camera_fixed {camera_fixed}: view indices must be in [0, {V})")
            self.cams = list(cams)  # (the refined cameras replace their entries: the caller's list stays as it is)
            self._view0 = torch.stack([c.view.detach().to(device="cpu", dtype=torch.float64) for c in cams])  # (V, 4, 4)
            self._xi = torch.zeros((V, 6), dtype=torch.float64)
            self._xi_grad = torch.zeros((V, 6), dtype=torch.float64)
            self._cam_opt = torch.optim.Adam([self._xi], lr=self.camera_lr)
            self._cam_host = {}  # view -> its (view, proj) as host float32 arrays (what the gr_views are built from)
            self._cam_rows = None  # the fused paths' per-step (len(my_views), 35) camera-gradient rows
            self._cam_params = {}  # the autograd path's pose leaves of this step
        self.exposure = bool(exposure)
        self.exposure_fused = bool(exposure_fused)
        if self.exposure_fused and not self.exposure:
            raise ValueError("exposure_fused without exposure: it selects the HIP device's form of exposure=True")
        self._expo_dev = False  # the fused path's exposure form runs (exposure_fused on the HIP device)
        if self.exposure:
            if self.dssim_fused:
                raise ValueError("exposure with dssim_fused: the fused D-SSIM form stages the colours inside its SSIM "
                                 "kernels and has no exposure (use dssim_fused=False)")
            if self.exposure_fused and self.w_dssim > 0.0:
                raise ValueError("exposure_fused with dssim_weight > 0: the fused exposure form has no D-SSIM term "
                                 "(gr_bwd_fit_exposure_gather is the L1 form's)")
            if dev.type == "cuda":
                if not self.exposure_fused:
                    raise ValueError("exposure on the HIP device: the fused fit path takes exposure only in its own form "
                                     "(pass exposure_fused=True / --exposure_fused), or fit on host tensors, --device cpu")
                self._exposure_check(dev)
                self._expo_dev = True
            V = len(cams)
            self.exposure_lr = float(exposure_lr)
            self.exposure_fixed = tuple(sorted({int(i) for i in exposure_fixed}))
            if any(not 0 <= i < V for i in self.exposure_fixed):
                raise ValueError(f"exposure_fixed {exposure_fixed}: view indices must be in [0, {V})")
            eye = torch.cat([torch.eye(3), torch.zeros(3, 1)], dim=1)
            self._expo = eye.repeat(V, 1, 1).to(device=dev, dtype=torch.float32).contiguous()  # (V, 3, 4)
            self._expo_grad = torch.zeros((V, 12), dtype=torch.float32, device=dev)  # d loss / d E of the last step
            self._expo_free = torch.ones((V, 1), dtype=torch.float32, device=dev)  # 0 on the rows of exposure_fixed
            for i in self.exposure_fixed:
                self._expo_free[i] = 0.0
            self._expo_opt = torch.optim.Adam([self._expo], lr=self.exposure_lr)
            self._expo_leaves = {}  # the exposure leaves of this step
            self._expo_rows = None  # the fused form's (V, 12) d loss / d E rows of this step (_views_scheduled)
        self._wgt_dev = False  # the fused path's weighted form runs (weights on the HIP device)
        if self.weights is not None:
            if self.w_dssim > 0.0:
                raise ValueError("weights with dssim_weight > 0: the weighted D-SSIM map is not built (the weights are the "
                                 "L1 terms')")
            if dev.type == "cuda":
                if self.exposure_fused:
                    raise ValueError("weights with exposure_fused: the fused exposure form has no loss weights "
                                     "(gr_bwd_fit_weighted_gather is the L1 form's); fit on host tensors, --device cpu")
                self._weights_check(dev)
                self._wgt_dev = True

    def canonical_params(self) -> dict:
        """The parameters in the stub's order (undoes the trainer's Morton permutation)."""
        self.graph_sync()
        if self.perm is None:
            return self.params
        out = {}
        for k, v in self.params.items():
            c = torch.empty_like(v.detach())
            c[self.perm] = v.detach()
            out[k] = torch.nn.Parameter(c)
        return out

    def respatialize(self) -> None:
        """Re-establish the Morton order of the Gaussians as they move during the fit: parameters and
        Adam moments are permuted in place (the optimizer keeps its state), self.perm follows."""
        if not self.reorder or self.params["means"].shape[0] < 2:
            return
        with torch.no_grad():
            p2 = morton_order(self.params["means"])
            for p in self.params.values():
                p.data.copy_(p.data[p2])
                st = self.opt.state.get(p)
                if st:
                    for k in ("exp_avg", "exp_avg_sq"):
                        if k in st:
                            st[k].copy_(st[k][p2])
            for b in self._stats:  # the density statistics are rows of the same Gaussians
                b.copy_(b[p2])
            self.perm = p2 if self.perm is None else self.perm[p2]

    def reset_optimizer(self) -> None:
        self.opt = torch.optim.Adam(list(self.params.values()), lr=self.lr)

    # ---- density statistics (density_stats=True) ----------------------------------------------------------------
    def _density_check(self, device) -> None:
        """On the HIP device the statistics come from the fused paths (gr_density_stats beside gr_reduce_sums): a fit
        that would take the per-view autograd path there has none, so it raises."""
        why = None
        if self.render_fn is not hip_render:
            why = "a custom render_fn"
        elif self.w_dssim > 0.0 and not self.dssim_fused:
            why = "dssim_weight > 0 without dssim_fused (the D-SSIM term on the autograd path)"
        elif not self._images_ok:
            why = "targets, masks or depths that are not exactly (height, width) float32 images"
        elif not all(p.dtype == torch.float32 for p in self.params.values()):
            why = "parameters that are not float32"
        elif not (FUSED_LOSS and DIRECT_BACKWARD and GATHER):
            why = "the fused path switched off (GR_FUSED_LOSS / GR_DIRECT / GR_GATHER)"
        if why is not None:
            raise ValueError(f"density_stats on {device}: the statistics come from the fused fit path only, which "
                             f"this fit does not take: {why}")

    def _exposure_check(self, device) -> None:
        """exposure_fused on the HIP device needs the fused path (_direct): a fit that would take the per-view autograd
        path there raises with the reason, as nothing falls back quietly."""
        why = None
        if self.render_fn is not hip_render:
            why = "a custom render_fn"
        elif not self._images_ok:
            why = "targets, masks or depths that are not exactly (height, width) float32 images"
        elif not all(p.dtype == torch.float32 for p in self.params.values()):
            why = "parameters that are not float32"
        elif not (FUSED_LOSS and DIRECT_BACKWARD):
            why = "the fused path switched off (GR_FUSED_LOSS / GR_DIRECT)"
        if why is not None:
            raise ValueError(f"exposure_fused on {device}: the exposure form is the fused fit path's, which this fit "
                             f"does not take: {why}")

    def _weights_check(self, device) -> None:
        """weights on the HIP device need the fused path (_direct): a fit that would take the per-view autograd path
        there raises with the reason, as nothing falls back quietly."""
        why = None
        if self.render_fn is not hip_render:
            why = "a custom render_fn"
        elif not self._images_ok:
            why = "targets, masks or depths that are not exactly (height, width) float32 images"
        elif not all(p.dtype == torch.float32 for p in self.params.values()):
            why = "parameters that are not float32"
        elif not (FUSED_LOSS and DIRECT_BACKWARD):
            why = "the fused path switched off (GR_FUSED_LOSS / GR_DIRECT)"
        if why is not None:
            raise ValueError(f"weights on {device}: the weighted form is the fused fit path's, which this fit does not "
                             f"take: {why}")

    def _loss_terms(self, depth: bool, ssim: bool = False) -> tuple:
        """A step's loss terms (w_sil, w_depth, g_scale, w_dssim) as every view path passes them on: the silhouette
        weight only with masks, the depth weight only with a depth term, the D-SSIM weight only in the D-SSIM form."""
        w_sil = self.w_sil if (self.masks is not None and self.w_sil > 0.0) else 0.0
        return w_sil, (self.w_depth if depth else 0.0), 1.0 / len(self.targets), (self.w_dssim if ssim else 0.0)

    def _inv_g_scale(self) -> float:
        """1 / g_scale of a step in float32, as gr_fit_views forms it: the schedules' statistics agree bit for bit."""
        return float(np.float32(1.0) / np.float32(1.0 / len(self.targets)))

    def _stats_bufs(self, ns: int, device) -> list:
        """The first ns streams' statistics buffers, zeroed when made (on the current stream: call before the render
        streams wait for it); kept until the Gaussian count changes."""
        n = int(self.params["means"].shape[0])
        if self._stats and (self._stats[0].shape[0] != n or self._stats[0].device != device):
            self._stats = []
        while len(self._stats) < ns:
            self._stats.append(torch.zeros((n, 2), dtype=torch.float32, device=device))
        return self._stats[:ns]

    def _cpu_sink(self, device):
        """cpu_renderer.capture_position_grads' sink: gr_density_stats' statistic from a render's d_px, d_py (the
        gradients of the step's loss, i.e. of the view loss / V).  A view sees a Gaussian whose position gradient is
        not zero (the dense render has no tiles to touch)."""
        buf = self._stats_bufs(1, device)[0]
        inv = float(len(self.targets))

        def sink(d_px, d_py, width, height):
            g = inv * torch.hypot(d_px * (0.5 * (width - 1)), d_py * (0.5 * (height - 1)))
            buf[:, 0] += g.to(buf.dtype)
            buf[:, 1] += ((d_px != 0) | (d_py != 0)).to(buf.dtype)

        return sink

    def density_state(self) -> tuple:
        """(gsum, seen) per Gaussian in canonical order (as canonical_params): the sum over the steps since the last
        densify and over the views that saw the Gaussian of the view loss's gradient norm w.r.t. its NDC x / y, and
        the number of those views.  The streams' buffers summed in stream order, then over the ranks (each saw its
        own views; a collective: every rank calls it)."""
        if not self.density_stats:
            raise ValueError("density_state: the fitter was made without density_stats")
        self.graph_sync()
        dev = self.params["means"].device
        n = int(self.params["means"].shape[0])
        bufs = [b for b in self._stats if b.shape[0] == n]
        tot = torch.zeros((n, 2), dtype=torch.float32, device=dev)
        for b in bufs:
            tot = tot + b
        if self.world > 1:
            dist.all_reduce(tot, group=self.group)
        if self.perm is not None:
            c = torch.empty_like(tot)
            c[self.perm] = tot
            tot = c
        return tot[:, 0].contiguous(), tot[:, 1].contiguous()

    # ---- camera pose refinement (refine_cameras=True) -----------------------------------------------------------
    def _cam_mats(self, i: int):
        """(view, proj) of view i as make_view takes them: while refining, host arrays kept with the refined poses (no
        device read per rebuilt gr_view); otherwise the camera's own tensors."""
        if not self.refine_cameras:
            return self.cams[i].view, self.cams[i].proj
        hit = self._cam_host.get(i)
        if hit is None:
            cam = self.cams[i]
            hit = self._cam_host[i] = (cam.view.detach().float().cpu().numpy().copy(),
                                       cam.proj.detach().float().cpu().numpy().copy())
        return hit

    def _camera_rows(self, count: int, device) -> torch.Tensor:
        """This step's camera-gradient rows, one per (virtual) view id of my_views, kept across steps."""
        r = self._cam_rows
        if r is None or r.shape[0] != max(1, count) or r.device != device:
            self._cam_rows = r = torch.zeros((max(1, count), tr._native.CAMERA_GRADS), dtype=torch.float32, device=device)
        return r

    def _camera_ws(self, k: int, n: int, device) -> torch.Tensor:
        """Render stream k's gr_camera_grads_sums workspace (reused in stream order)."""
        ws = self._cam_ws
        need = max(8, int(tr._native.lib().gr_camera_grads_ws_bytes(n, tr._native.REDUCE_MAX_VIEWS)))
        t = ws.get(k)
        if t is None or t.numel() < need or t.device != device:
            ws[k] = t = torch.empty((need,), dtype=torch.uint8, device=device)
        return t

    def _camera_grads_batch(self, m, s, c, o, batch, js, k: int) -> None:
        """gr_camera_grads_sums of a reduction batch on the current stream: batch entry q is view js[q] of my_views."""
        rows = self._camera_rows(len(self.my_views), m.device)
        tr.camera_grads_sums_native(m, s, c, o, batch, [rows[j] for j in js], ws=self._camera_ws(k, int(m.shape[0]), m.device))

    def _camera_step_fused(self, device) -> None:
        """After a fused step's streams joined: the rows of this rank's (virtual) views added per real view in my_views'
        order (a view's bands add up), summed over the ranks, and the pose update on the host."""
        V = len(self.targets)
        views = self.my_views
        tot = torch.zeros((V, tr._native.CAMERA_GRADS), dtype=torch.float32, device=device)
        if views:
            rows = self._camera_rows(len(views), device)
            for j, i in enumerate(views):
                tot[self._vi(i)] += rows[j]
        if self.world > 1:
            dist.all_reduce(tot, group=self.group)
        if device.type == "cuda":
            pin = self._cam_pin
            if pin is None or pin.shape != tot.shape:
                self._cam_pin = pin = torch.empty(tot.shape, dtype=torch.float32, pin_memory=True)
            pin.copy_(tot, non_blocking=True)
            torch.cuda.current_stream(device).synchronize()
            tot = pin
        self._camera_update(self._camera_xi_grad(tot))

    def _camera_xi_grad(self, rows: torch.Tensor) -> torch.Tensor:
        """(V, 35) host rows (gr_bwd_camera's layout, one per view) -> d loss / d xi (V, 6) float64: d view completed
        with the camera centre's term (torch_renderer._camera_grads), then the vector-Jacobian product through
        pose_view, all views in one pass."""
        sh = "colors_raw" not in self.params
        dview = torch.stack([tr._camera_grads(rows[i], torch.from_numpy(self._cam_mats(i)[0]), None,
                                              True, False, sh)[0].double() for i in range(rows.shape[0])])
        xi = self._xi.detach().clone().requires_grad_(True)
        (g,) = torch.autograd.grad((pose_view(xi, self._view0) * dview).sum(), xi)
        return g

    def _camera_leaf(self, i: int, device):
        """The autograd path: view i's camera with its view matrix a function of a pose leaf of this step."""
        xi = self._xi[i].detach().clone().requires_grad_(True)
        self._cam_params[i] = xi
        view = pose_view(xi, self._view0[i]).to(device=device, dtype=self.cams[i].view.dtype)
        return tr.Camera(view=view, proj=self.cams[i].proj)

    def _camera_step_autograd(self) -> None:
        """After the autograd path's backward: d loss / d xi of this rank's views, summed over the ranks, the update."""
        V = len(self.targets)
        g = torch.zeros((V, 6), dtype=torch.float64)
        for i, xi in self._cam_params.items():
            if xi.grad is not None:
                g[i] = xi.grad
        self._cam_params = {}
        if self.world > 1:
            dev = self.params["means"].device
            t = g.to(dev)
            dist.all_reduce(t, group=self.group)
            g = t.cpu()
        self._camera_update(g)

    def _camera_update(self, g: torch.Tensor) -> None:
        """Adam on the pose deltas from the all-reduced d loss / d xi (every rank the same arithmetic on the same
        numbers), the rows of camera_fixed left alone; then the cameras and everything built from their matrices."""
        for i in self.camera_fixed:
            g[i] = 0.0
        self._xi_grad = g.clone()
        self._xi.grad = g
        self._cam_opt.step()
        self._xi.grad = None
        with torch.no_grad():
            dev = self.params["means"].device
            v32 = pose_view(self._xi, self._view0).to(torch.float32)  # formed in float64, rounded once
            vdev = v32.to(dev)  # (one copy; the cameras' views are its rows)
            vnp = v32.numpy()
            for i, cam in enumerate(self.cams):
                if i in self.camera_fixed:  # (a gradient that is always zero: Adam leaves the row at zero)
                    continue
                self.cams[i] = tr.Camera(view=vdev[i].to(cam.view.dtype), proj=cam.proj)
                if i in self._cam_host:
                    self._cam_host[i] = (vnp[i], self._cam_host[i][1])
        # the gr_views that hold the matrices are rebuilt on their next use (band cuts keep their refresh points)
        self._drop_views()

    def refined_cameras(self) -> list:
        """The cameras at their current poses, in the fitter's view order."""
        self.graph_sync()
        return list(self.cams)

    def camera_state(self) -> tuple:
        """(xi, d loss / d xi of the last step), both (V, 6) float64 on the host: the pose deltas (pose_view) and the
        gradient the last update used (rows of camera_fixed zero)."""
        if not self.refine_cameras:
            raise ValueError("camera_state: the fitter was made without refine_cameras")
        return self._xi.detach().clone(), self._xi_grad.clone()

    # ---- exposure compensation (exposure=True) ------------------------------------------------------------------
    def _exposure_leaf(self, i: int) -> torch.Tensor:
        """View i's exposure as a leaf of this step."""
        e = self._expo[i].detach().clone().requires_grad_(True)
        self._expo_leaves[i] = e
        return e

    def _exposure_step_autograd(self) -> None:
        """After the step's backward: d loss / d E of this rank's views, summed over the ranks, the update."""
        V = len(self.targets)
        g = torch.zeros((V, 12), dtype=torch.float32, device=self._expo.device)
        for i, e in self._expo_leaves.items():
            if e.grad is not None:
                g[i] = e.grad.reshape(12)
        self._expo_leaves = {}
        if self.world > 1:
            dist.all_reduce(g, group=self.group)
        self._exposure_update(g)

    def _exposure_step_fused(self) -> None:
        """_exposure_step_autograd for the fused path's exposure form: the step's (V, 12) rows as the views' kernels
        wrote them (this rank's; zero elsewhere), on the main stream after it has waited for the render streams.  No host
        read: the rows, the all-reduce and the update stay on the device."""
        g, self._expo_rows = self._expo_rows, None
        if self.world > 1:
            dist.all_reduce(g, group=self.group)
        self._exposure_update(g)

    def _exposure_update(self, g: torch.Tensor) -> None:
        """Adam on the exposures from the all-reduced (V, 12) gradient (every rank the same arithmetic on the same
        numbers), the rows of exposure_fixed zeroed: a gradient that is always zero leaves its row where it is."""
        g = g * self._expo_free
        self._expo_grad = g
        self._expo.grad = g.view(-1, 3, 4)
        self._expo_opt.step()
        self._expo.grad = None

    def exposure_state(self) -> tuple:
        """(E, d loss / d E of the last step), both (V, 3, 4) float32 on the host, in the fitter's view order (rows of
        exposure_fixed: E as it started, a zero gradient)."""
        if not self.exposure:
            raise ValueError("exposure_state: the fitter was made without exposure")
        self.graph_sync()
        return self._expo.detach().cpu().clone(), self._expo_grad.detach().cpu().reshape(-1, 3, 4).clone()

    def set_exposures(self, E) -> None:
        """Replace every view's exposure matrix: (V, 3, 4), e.g. `exposure` of an earlier fit's exposures.npz (the rows
        of exposure_fixed too: they stay where this puts them).  The exposure Adam's moments are kept."""
        if not self.exposure:
            raise ValueError("set_exposures: the fitter was made without exposure")
        E = torch.as_tensor(E, dtype=torch.float32)
        if tuple(E.shape) != tuple(self._expo.shape):
            raise ValueError(f"set_exposures: expected shape {tuple(self._expo.shape)}, got {tuple(E.shape)}")
        self.graph_sync()
        with torch.no_grad():
            self._expo.copy_(E.to(self._expo.device))

    def _background(self, device) -> torch.Tensor:
        # one persistent tensor: the renderer reads its value on the host once, not per view
        if self._bg is None or self._bg.device != device:
            self._bg = torch.zeros(3, device=device)
        return self._bg

    @property
    def my_views(self) -> list:
        """This rank's views: i = r, r + R, ... (whole views), or with band splitting the first R * (V // R) views
        round-robin and this rank's band of its group's leftover view (a virtual id V + i, _vi / _bands)."""
        if not self._bands_ok():
            return self._rr_views
        V, W = len(self.targets), self.world
        q = V // W
        whole = list(range(self.rank, q * W, W))
        band = self._band_of(self.rank)
        if band is None:  # (more ranks in the group than the view has tile rows: this rank renders no band)
            return whole
        i, lo, rows = band
        self._bands[V + i] = band
        return whole + [V + i]

    def _band_groups(self) -> list:
        """[(leftover view, first rank, ranks)]: the R ranks in r = V mod R contiguous groups, one per leftover view."""
        V, W = len(self.targets), self.world
        r = V % W
        return [(V - r + j, j * W // r, (j + 1) * W // r - j * W // r) for j in range(r)]

    def _band_of(self, rank: int):
        """(view, first tile row, tile rows) of `rank`'s band, or None (its group's view has fewer tile rows than ranks)."""
        for i, r0, g in self._band_groups():
            if r0 <= rank < r0 + g:
                cuts = self._band_cuts(i, g)
                k = rank - r0
                return (i, cuts[k], cuts[k + 1] - cuts[k]) if cuts[k + 1] > cuts[k] else None
        return None

    def _band_cuts(self, i: int, g: int) -> list:
        """Tile-row boundaries cutting view i into g bands of about equal work: a band's time is a fixed part plus its
        (Gaussian, tile) pairs (tools/band_probe.py: ~90 us + ~130 us per million pairs at C4, single stream), and a
        scene's pairs crowd the middle rows (view 48 of C4: rows 6-18 of 25 hold 97% of them), so equal rows left the
        middle bands twice the edge ones' work.  The pairs per row are estimated from the Gaussians' projected 5-sigma
        boxes (rows x tile columns touched), recomputed with the Morton re-sort and after densify; every rank computes
        the same cuts from its identical replica."""
        tile = self.views_tile()
        ty = -(-self.height // tile)
        key = (i, g, tile, int(self.params["means"].shape[0]), self.steps_done // max(1, RESORT_EVERY))
        cache = self._cuts_cache
        if key in cache:
            return cache[key]
        if len(cache) > 64:
            cache.clear()
        w = self._row_pairs_cached(i, tile, ty)
        cuts = _min_max_cuts(w, g) if ty >= g else [ty * k // g for k in range(g + 1)]
        cache[key] = cuts
        return cuts

    def _row_pairs_cached(self, i: int, tile: int, ty: int) -> np.ndarray:
        key = (i, tile, int(self.params["means"].shape[0]), self.steps_done // max(1, RESORT_EVERY))
        cache = self._rows_cache
        if key not in cache:
            if len(cache) > 64:
                cache.clear()
            cache[key] = self._row_pairs(i, tile, ty)
        return cache[key]

    def _row_pairs(self, i: int, tile: int, ty: int) -> np.ndarray:
        """Estimated (Gaussian, tile) pairs per tile row of view i: per Gaussian the tile rows and columns of its
        FIT_CUTOFF-sigma box (torch_renderer.py:57-78, 146-150's projection and sigma rule; rectangle, not the
        elliptical test), summed over the rows it spans (a difference array)."""
        with torch.no_grad():
            m, sc, _, _ = activations(self.params)
            cam = self.cams[i]
            V, P = cam.view.float(), cam.proj.float()
            pc = m.float() @ V[:3, :3].T + V[:3, 3]
            clip = pc @ P[:3, :3].T + P[:3, 3]
            w4 = pc @ P[3, :3] + P[3, 3]
            ws = torch.where(w4.abs() < 1e-8, torch.ones_like(w4), w4)
            ndc = clip / ws[:, None]
            ok = (ndc[:, 2] >= -1) & (ndc[:, 2] <= 1) & (w4 != 0)
            px = (ndc[:, 0] * 0.5 + 0.5) * (self.width - 1)
            py = (1 - (ndc[:, 1] * 0.5 + 0.5)) * (self.height - 1)
            za = pc[:, 2].abs().clamp_min(1e-6)
            sx = (sc[:, 0].abs() * 0.5 * self.width * P[0, 0].abs() / za).clamp_min(1.0) * tr.FIT_CUTOFF
            sy = (sc[:, 1].abs() * 0.5 * self.height * P[1, 1].abs() / za).clamp_min(1.0) * tr.FIT_CUTOFF
            tx = -(-self.width // tile)
            c0 = ((px - sx) / tile).floor().clamp(0, tx - 1)
            c1 = ((px + sx) / tile).floor().clamp(0, tx - 1)
            r0 = ((py - sy) / tile).floor().clamp(0, ty - 1)
            r1 = ((py + sy) / tile).floor().clamp(0, ty - 1)
            ok = ok & (px + sx >= 0) & (px - sx <= self.width - 1) & (py + sy >= 0) & (py - sy <= self.height - 1)
            cols = torch.where(ok, c1 - c0 + 1, torch.zeros_like(c0)).long()
            # a difference array of integer counts, summed without atomics (a sort, a prefix sum and a search): exact
            # and the same on every rank (an index_add_ of float64 took 28 ms per view at C4)
            d = _int_hist(r0.long(), cols, ty + 1) - _int_hist((r1 + 1).long(), cols, ty + 1)
            return torch.cumsum(d, 0)[:ty].double().cpu().numpy()

    def views_tile(self) -> int:
        """The tile size the fused path renders this fit's views at: FIT_TILE, or 16 in the f32-grade mode (its
        three-piece splits have 16-pixel kernels only)."""
        return (16 if F32_GRADE else FIT_TILE) or 16

    def _ssim_form(self) -> bool:
        """The fused path runs its D-SSIM form (dssim_fused with a D-SSIM term): whole views with 16-pixel tiles, the
        per-view schedule only (no batched / graph step, no tile-row bands: an SSIM window crosses band rows)."""
        return self.dssim_fused and self.w_dssim > 0.0

    def _bands_ok(self) -> bool:
        if self._ssim_form() or self._expo_dev or self._wgt_dev:  # (the exposure and weighted forms: whole views
            return False                                            # through their gather entries)
        V, W = len(self.targets), self.world
        r = V % W if W > 1 else 0
        if not (BAND_SPLIT and r and not self._depth_grad()):
            return False
        if self.params["means"].shape[0] == 0:  # (the generic loop renders whole views only)
            return False
        dev = self.params["means"].device
        if not (dev.type == "cuda" and self._direct(dev)):
            return False
        # the most loaded rank: V // R views and one band, its largest share of its view's pairs plus the band's fixed
        # cost (a group of one renders its whole view, no band cost): bands only where that beats a whole view
        load = max((1.0 if g == 1 else BAND_OVERHEAD + self._band_share(i, g)) for i, _, g in self._band_groups())
        return load < 1.0

    def _band_share(self, i: int, g: int) -> float:
        """The largest band's share of view i's estimated pairs when cut into g bands (_band_cuts)."""
        tile = self.views_tile()
        w = self._row_pairs_cached(i, tile, -(-self.height // tile))
        cuts = self._band_cuts(i, g)
        tot = float(w.sum())
        return max(float(w[cuts[k]:cuts[k + 1]].sum()) for k in range(g)) / tot if tot > 0 else 1.0 / g

    def _vi(self, v: int) -> int:
        """The view index of a (possibly virtual, band) view id."""
        return v - len(self.targets) if v >= len(self.targets) else v

    def _depth_grad(self) -> bool:
        """The loss differentiates the depth output (a depth term): the views render in the default
        precision mode with the depth-gradient cutoff; otherwise depth_grad=False (gr_view.no_depth_grad)."""
        return self.depths is not None and self.w_depth > 0.0

    def _prepare(self, i: int, means, scales, colors, opacities, fit_view: bool = False, plan_host=None):
        """fit_view: a view of the fused path (_views_direct): one zone at tr.FIT_CUTOFF."""
        cam = self.cams[i]
        cut = tr.FIT_CUTOFF if fit_view else None
        return tr.prepare_view(means, scales, colors, opacities, cam.view, cam.proj, self.width, self.height,
                               self._background(means.device), cutoff=cut,
                               core_cutoff=tr.FIT_CUTOFF if fit_view else tr.DEFAULT_CORE_CUTOFF,
                               depth_grad="eager" if self._depth_grad() else False, plan_host=plan_host)

    @staticmethod
    def _prep_groups(views, ahead: dict, prepare_views: Callable, prep) -> Callable[[int], None]:
        """prepare_upto(j): the views up to j prepared on stream `prep` (whole groups, in order: the first
        PREP_FIRST views, then PREP_GROUP at a time; their states go to `ahead`).  Called with the first two
        groups at once, then after each render (its j + PREP_AHEAD): the step's first render is launched
        before the host spends time on later groups (a 7-view step waited ~180 us for them)."""
        nxt = [0]

        def prepare_upto(j):
            while nxt[0] <= j and nxt[0] < len(views):
                j0 = nxt[0]
                js = range(j0, min(len(views), j0 + (PREP_FIRST if j0 == 0 else PREP_GROUP)))
                with torch.cuda.stream(prep):
                    ahead.update(zip(js, prepare_views(js)))
                nxt[0] = js.stop

        prepare_upto(min(PREP_FIRST, PREP_AHEAD - 1) if PREP_INITIAL > 1 else 0)
        return prepare_upto

    def _gr_view(self, kind: str, i, device) -> "tr._native.GrView":
        """The one cache of gr_views, each built once: cameras and background change during a fit only through
        _camera_update, which drops them all (_drop_views).  Building one costs the host a matrix inverse and copies.
          fit    view i for the fused path: one FIT_CUTOFF zone, no depth gradient, FIT_TILE tiles (F32_GRADE: the
                 f32-grade mode on 16-pixel tiles); keyed by those two switches as well
          ssim   the same with 16-pixel tiles, the SSIM kernels' tile (the D-SSIM form without a depth term)
          depth  view i in the default precision mode with the depth gradient's footprint (a depth term)
          band   a band id i >= V (_bands): its view's `fit` view cut to the band's tile rows; keyed by the cut too
          eval   the view render_gaussians_torch(..., depth_grad=False) makes for camera object i with the fitter's
                 background (16-pixel tiles, default_cutoff(False), the default core cutoff); keyed by the object's
                 identity, and the object is kept with the view so that the identity stays its own"""
        if kind == "eval":
            key = (kind, id(i), str(device))
            hit = self._gv.get(key)
            if hit is None:
                hit = self._gv[key] = (tr.make_view(i.view, i.proj, self.width, self.height, self._background(device),
                                                    depth_grad=False), i)
            return hit[0]
        if kind == "depth":
            key = (kind, i)
        elif kind == "ssim":
            key = (kind, i, F32_GRADE)
        else:
            key = (kind, i, F32_GRADE, FIT_TILE) + (self._bands[i] if kind == "band" else ())
        gv = self._gv.get(key)
        if gv is not None:
            return gv
        if kind == "band":
            base, row0, rows = self._bands[i]
            gv = tr._native.GrView.from_buffer_copy(self._gr_view("fit", base, device))
            gv.row0, gv.rows = row0, rows
        elif kind == "depth":
            gv = tr.make_view(*self._cam_mats(i), self.width, self.height, self._background(device), depth_grad=True)
        else:
            tile = {} if kind == "ssim" else {"tile": 0 if F32_GRADE else FIT_TILE}
            gv = tr.make_view(*self._cam_mats(i), self.width, self.height, self._background(device),
                              cutoff=tr.FIT_CUTOFF, core_cutoff=tr.FIT_CUTOFF, depth_grad=False, **tile)
            if F32_GRADE:
                gv.no_depth_grad = 2
        self._gv[key] = gv
        return gv

    def _drop_views(self) -> None:
        """The cameras' matrices changed: every gr_view, and the executor's target array that holds copies of them, is
        rebuilt on its next use (band cuts keep their refresh points)."""
        self._gv.clear()
        self._native_targets = None

    def _fit_view(self, i: int, device) -> "tr._native.GrView":
        """The fused path's gr_view of view i, or of band id i >= V (_gr_view's `fit` / `band`)."""
        return self._gr_view("band" if i >= len(self.targets) else "fit", i, device)

    def _ssim_view(self, i: int, device) -> "tr._native.GrView":
        """The gr_view of view i for the fused path's D-SSIM form without a depth term (_gr_view's `ssim`)."""
        return self._gr_view("ssim", i, device)

    def _step_view(self, i: int, device, depth: bool, ssim: bool = False) -> "tr._native.GrView":
        """The gr_view the fused step renders (virtual) view i with, in every schedule."""
        if depth:
            return self._gr_view("depth", i, device)
        return self._ssim_view(i, device) if ssim else self._fit_view(i, device)

    def _plan_pins(self, count: int) -> torch.Tensor:
        """One pinned (count, 3) int64 buffer for the views' plans, kept across steps (a pinned allocation
        per view and step costs host time on the render path)."""
        pins = self._pins
        if pins is None or pins.shape[0] < count:
            self._pins = pins = torch.zeros((max(count, 1), 3), dtype=torch.int64, pin_memory=True)
        return pins

    def view_loss(self, i: int, means, scales, colors, opacities, prepared=None) -> torch.Tensor:
        device = means.device
        kw = {} if prepared is None else {"prepared": prepared}
        if self.render_fn is hip_render:
            # without a depth loss the depth output gets no gradient: the forward may accumulate W and D
            # at the colours' precision (gr_view.no_depth_grad)
            kw["depth_grad"] = "eager" if self._depth_grad() else False  # a depth loss differentiates depth
        cam = self._camera_leaf(i, device) if self.refine_cameras and torch.is_grad_enabled() else self.cams[i]
        pred, alpha, depth = self.render_fn(means, scales, colors, opacities, cam, self.width, self.height,
                                            self._background(device), **kw)
        use_sil = self.masks is not None and self.w_sil > 0.0
        if self.exposure:
            # the photometric term (L1 and D-SSIM alike) compares the exposed colour pred @ E[:, :3].T + E[:, 3] with
            # the target: formed channel by channel (element-wise products and sums, whose backward reduces over the
            # pixels; as a matrix product its backward would be a (3, HW) x (HW, 3) BLAS call per view) and kept in the
            # render's own memory layout (the loss's reductions then sum in the order they have without exposure, and
            # identity E gives that fit's bits)
            E = self._exposure_leaf(i).to(pred.device)
            y = pred[..., 0:1] * E[:, 0] + pred[..., 1:2] * E[:, 1] + pred[..., 2:3] * E[:, 2] + E[:, 3]
            pred = torch.empty_like(pred).copy_(y)
        wgt = None if self.weights is None else self.weights[i]
        if wgt is not None:
            # every L1 term of pixel p times its weight, the means over all 3 HW / HW elements (ones: the same bits)
            loss = torch.mean(wgt[..., None] * torch.abs(pred - self.targets[i]))
            if use_sil:
                loss = loss + self.w_sil * torch.mean(wgt * torch.abs(alpha - self.masks[i]))
        elif self.w_dssim > 0.0:
            # (1 - l) L1 + l D-SSIM for the photometric term; the silhouette term as below
            lam = self.w_dssim
            if self.render_fn is hip_render and pred.device.type == "cuda" and FUSED_LOSS:
                loss = (1.0 - lam) * losses.l1_loss(pred, self.targets[i]) + lam * losses.dssim_loss(pred, self.targets[i])
                if use_sil:
                    loss = loss + self.w_sil * losses.l1_loss(alpha, self.masks[i])
            else:
                loss = (1.0 - lam) * torch.mean(torch.abs(pred - self.targets[i])) + lam * losses.dssim_loss(pred, self.targets[i])
                if use_sil:
                    loss = loss + self.w_sil * torch.mean(torch.abs(alpha - self.masks[i]))
        elif self.render_fn is hip_render and pred.device.type == "cuda" and FUSED_LOSS:
            # photometric + silhouette L1 fused on the device (losses.l1_loss); same value and gradient
            loss = losses.l1_loss(pred, self.targets[i], alpha if use_sil else None,
                                  self.masks[i] if use_sil else None, self.w_sil if use_sil else 0.0)
        else:
            loss = torch.mean(torch.abs(pred - self.targets[i]))
            if use_sil:
                loss = loss + self.w_sil * torch.mean(torch.abs(alpha - self.masks[i]))
        if self.depths is not None and self.w_depth > 0.0:
            d_pred = depth / (depth.max() + 1e-6)
            if wgt is not None:  # (the maximum over all pixels, unweighted: autograd gives its weighted chain term)
                loss = loss + self.w_depth * torch.mean(wgt * torch.abs(d_pred - self.depths[i]))
            else:
                loss = loss + self.w_depth * torch.mean(torch.abs(d_pred - self.depths[i]))
        return loss

    # ---- the fused path's streams, kept buffers and its one per-view schedule ------------------------------------
    def _streams(self, device, ns: int) -> tuple:
        """(the ns - 1 render streams besides the caller's, the preparation stream): the fitter's own, shared by the
        fit step in every form, the native executor's calls, evaluate() and contribution_state().  The side streams
        are made before the preparation stream, and that one at PREP_PRIORITY: creation order decides the streams'
        hardware-queue placement.  More side streams are made only when too few exist, and none is ever dropped: a
        call over fewer views than the fit has streams (an evaluate() of two held-out views) uses the first of them and
        leaves the fit's streams as they are.  (Before, any call with another stream count re-created them all.)"""
        if (self._side and self._side[0].device != device) or (self._prep is not None and self._prep.device != device):
            self._side, self._prep = [], None
        while len(self._side) < ns - 1:
            self._side.append(torch.cuda.Stream(device))
        if self._prep is None:
            self._prep = torch.cuda.Stream(device, priority=PREP_PRIORITY)
        return self._side[:max(0, ns - 1)], self._prep

    def _acc_sets(self, owner: str, ns: int, m, s, c, o) -> tuple:
        """(ns stream accumulator sets, each four tensors like m, s, c, o; their 4 * ns pointers as the executor takes
        them), kept per owner ("direct": the Python and batched schedules, "native": the executor) while the shapes
        hold: 4 x streams allocations per step were host time before the first launch.  They are written only after
        the render streams wait for the caller's stream, i.e. after the previous step's parameter update read them."""
        shapes = (ns,) + tuple(tuple(t.shape) for t in (m, s, c, o))
        kept = self._acc_kept.get(owner)
        if kept is None or kept[0] != shapes or kept[1][0][0].device != m.device:
            acc = [tuple(torch.empty_like(t) for t in (m, s, c, o)) for _ in range(ns)]
            self._acc_kept[owner] = kept = (shapes, acc, (ctypes.c_void_p * (4 * ns))(*[t.data_ptr() for a in acc for t in a]))
        return kept[1], kept[2]

    def _exec_config(self, device, ns: int, sized=None) -> "tr._native.GrFitConfig":
        """The native executor's configuration of a call over ns streams: the module's schedule knobs, with `sized`
        the device-side sizing state (capacities, observed counts, overflow word), and the fitter's own torch streams
        (EXEC_STREAMS): the same hardware-queue placement as the Python schedule, so the two differ only in their
        host code."""
        cfg = tr._native.GrFitConfig(NUM_STREAMS, PREP_AHEAD, PREP_GROUP, PREP_FIRST, REDUCE_BATCH, min(REDUCE_TAIL, REDUCE_BATCH))
        if sized is not None:
            cfg.caps = sized.caps_arr
            cfg.observed = sized.observed.data_ptr()
            cfg.overflow = sized.ovf.data_ptr()
        if EXEC_STREAMS:
            side, prep = self._streams(device, ns)
            self._exec_streams = rs = (ctypes.c_void_p * max(1, ns - 1))(*[st.cuda_stream for st in side])
            cfg.render_streams = rs
            cfg.prep_stream = prep.cuda_stream
        return cfg

    def _reg_after_exec(self, reg_fn, device):
        """The regulariser's small kernels after the executor's call (the host starts the views' preparations first),
        on the preparation stream behind the last preparation when the executor runs on the fitter's streams (as the
        Python schedule does; no extra hardware queue).  Returns reg_fn()'s value, or None."""
        if reg_fn is None:
            return None
        prep = self._prep if EXEC_STREAMS else None
        if prep is None:
            return reg_fn()
        main = torch.cuda.current_stream(device)
        with torch.cuda.stream(prep):
            reg = reg_fn()
        reg.record_stream(main)  # allocated on prep, read on main: not reused by prep early
        main.wait_stream(prep)
        return reg

    def _preparer(self, m, s, c, o, gv_at: Callable, count: int, sized=None) -> Callable:
        """_view_loop's preparation callable over positions 0 .. count - 1 (gv_at(q): position q's gr_view): host-sized
        (the plans land in pinned rows the forward reads), or with `sized` (_graph_step) device-sized: capacities in,
        the true counts to the pinned `observed` rows."""
        if sized is None:
            pins = self._plan_pins(count)
            return lambda js: tr.prepare_views_native(m, s, c, o, [gv_at(q) for q in js], [pins[q] for q in js])
        return lambda js: tr.prepare_views_sized(m, s, c, o, [tr.sized_view(gv_at(q)) for q in js],
                                                 [sized.caps[q] for q in js], [sized.observed[q] for q in js], sized.ovf)

    def _view_loop(self, device, count: int, prepare_views: Callable, body: Callable, reduce: Optional[Callable] = None,
                   tail_fn: Optional[Callable] = None):
        """The fused path's per-view schedule, the one every Python form runs (the L1, depth and D-SSIM fit steps,
        evaluate(), contribution_state()) and the native executor mirrors (gr_fit_exec.cpp):
          * the preparation groups (_prep_groups over prepare_views) run PREP_AHEAD views ahead on the preparation stream;
          * view j runs on render stream j % ns (the caller's stream first): the stream waits for the prepared view's
            event, its geometry is recorded on the stream, then body(j, take) runs with the stream current.  The body
            takes the prepared view with take(j): the loop itself keeps no reference to it or to anything the body
            makes, so each body decides when its memory returns to the allocator;
          * with `reduce`, what the bodies return waits per stream in view order and is reduced in the batches of
            _batch_sizes: reduce(k, batch, js, accumulate) on stream k, js the batch's positions, accumulate False
            for a stream's first batch;
          * tail_fn() runs on the preparation stream after the last preparation (its tensor recorded on the caller's);
          * the caller's stream waits for every render stream, then for the preparation stream.
        Three ordering rules carry the bit-identity with the executor and must hold for every caller:
          1. whatever the bodies write (losses, accumulators, statistics, camera rows) is allocated on the caller's
             stream before this is called: the render streams' first act is to wait for that stream;
          2. kept accumulators are therefore written only after the previous parameter update read them;
          3. a stream's reductions run in view order, and the caller sums the streams in stream order.
        Returns tail_fn()'s value (None without one)."""
        main = torch.cuda.current_stream(device)
        ns = max(1, min(NUM_STREAMS, count))
        side, prep = self._streams(device, ns)
        streams = [main] + side
        for st in side:
            st.wait_stream(main)
        prep.wait_stream(main)
        ahead: dict = {}
        take = ahead.pop
        prepare_upto = self._prep_groups(range(count), ahead, prepare_views, prep)
        pending: list = [[] for _ in streams]  # per stream: what its bodies returned, awaiting their reduction
        pending_js: list = [[] for _ in streams]  # their positions (the camera-gradient rows)
        started = [False] * ns
        sizes = _batch_sizes(ns, count) if reduce is not None else None

        def reduce_pending(k):
            if pending[k]:
                with torch.cuda.stream(streams[k]):
                    reduce(k, pending[k], pending_js[k], started[k])
                started[k] = True
                pending[k] = []
                pending_js[k] = []

        for j in range(count):
            k = j % ns
            st = streams[k]
            prepare_upto(j)
            pv = ahead[j]
            st.wait_event(pv.event)
            pv.geom.record_stream(st)
            pv = None
            with torch.cuda.stream(st):
                item = body(j, take)
            prepare_upto(j + PREP_AHEAD)
            if reduce is not None:
                pending[k].append(item)
                pending_js[k].append(j)
                item = None
                if len(pending[k]) >= sizes[k][0]:
                    reduce_pending(k)
                    if len(sizes[k]) > 1:
                        sizes[k].pop(0)
        if reduce is not None:
            for k in range(ns):
                reduce_pending(k)
        tail = None
        if tail_fn is not None:
            with torch.cuda.stream(prep):
                tail = tail_fn()
                if isinstance(tail, torch.Tensor):
                    tail.record_stream(main)  # allocated on the preparation stream, read on main
        for st in side:
            main.wait_stream(st)
        main.wait_stream(prep)
        return tail

    def _reduce_batch(self, m, s, c, o, batch, js, k: int, acc, stats, accumulate: bool, gathered: bool = True) -> None:
        """One reduction batch of render stream k, on the current stream: the chain rules from the views' gathered
        sums into the stream's accumulator set (gr_reduce_sums), with density_stats the statistics beside it, with
        refine_cameras the camera gradients after it (batch entry q is position js[q] of my_views).  gathered False
        (the L1 form with GR_GATHER=0): the one-pass gr_reduce_views over the views' kept workspaces."""
        if not gathered:
            if self.refine_cameras:
                raise ValueError("refine_cameras: the fused path's camera gradient reads the gathered sums "
                                 "(GR_GATHER=0 has none)")
            tr.reduce_views_native(m, s, c, o, batch, acc[k], accumulate=accumulate)
            return
        tr.reduce_sums_native(m, s, c, o, batch, acc[k], accumulate=accumulate)
        if stats is not None:
            tr.density_stats_native(m, s, o, batch, self._inv_g_scale(), stats[k])
        if self.refine_cameras:
            self._camera_grads_batch(m, s, c, o, batch, js, k)

    def _form(self) -> str:
        """The fused step's form: "exposure" (exposure_fused, with or without a depth term), "weighted" (weights, with
        or without a depth term), "ssim" (the D-SSIM form, with or without a depth term), "depth" or "l1"."""
        if self._expo_dev:
            return "exposure"
        if self._wgt_dev:
            return "weighted"
        return "ssim" if self._ssim_form() else "depth" if self._depth_grad() else "l1"

    def _direct(self, device) -> bool:
        """The fused path (_views_direct, or _views_scheduled's depth and D-SSIM forms): HIP render op, the
        view loss and its gradients in the C ABI, no autograd per view.  Needs float32 parameters and
        targets / masks / depths of exactly the image's shape (checked at construction).  A D-SSIM term
        (dssim_weight > 0) is not fused into the splat epilogues: such a fit takes the per-view autograd path, or with
        dssim_fused the fused path's D-SSIM form (_ssim_form)."""
        if self.w_dssim > 0.0 and not self.dssim_fused:
            return False
        return (self.render_fn is hip_render and device.type == "cuda" and FUSED_LOSS and DIRECT_BACKWARD
                and self._images_ok and all(p.dtype == torch.float32 for p in self.params.values()))

    def step(self) -> torch.Tensor:
        """One iteration; returns the full (all-rank) loss as a 0-d tensor on the device."""
        if RESORT_EVERY and self.steps_done and self.steps_done % RESORT_EVERY == 0:
            self.respatialize()
        self.steps_done += 1
        device = self.params["means"].device
        if self._graph_ok(device):
            return self._graph_step(device)
        self._graph_leave()
        self.opt.zero_grad(set_to_none=True)
        if self._direct(device) and self.params["means"].shape[0] > 0 and self._fused_step_ok():
            with torch.no_grad():
                means, scales, colors, opacities, reg_t = self._activations_fused(device)
                total, reg = self._views_fused(means, scales, colors, opacities, reg_t, self._native_exec() and GATHER)
                loss = total / len(self.targets)
                if reg is not None:
                    loss = loss + reg
            out = self._fused_param_step(scales, opacities, loss)
            if self.refine_cameras:  # the next step renders with this update
                self._camera_step_fused(device)
            if self._expo_dev:
                self._exposure_step_fused()
            return out
        means, scales, colors, opacities = activations(self.params)
        if self._direct(device) and means.shape[0] > 0:
            total, _ = self._views_scheduled(means, scales, colors, opacities, self._form())
            parts = self._acc_parts
            acc = []
            for q in range(4):  # in stream order
                t = parts[0][q]
                for pp in parts[1:]:
                    t = t + pp[q]
                acc.append(t)
            self._acc = tuple(acc)
            loss = total / len(self.targets)
            if self.rank == 0:
                reg = self.reg_opacity * opacities.mean() + self.reg_scale * scales.mean()
                loss = loss + reg.detach()
                torch.autograd.backward([means, scales, colors, opacities, reg], list(self._acc) + [None])
            else:
                torch.autograd.backward([means, scales, colors, opacities], list(self._acc))
            self._acc = None
            out = self._finish_step(loss)
            if self.refine_cameras:
                self._camera_step_fused(device)
            if self._expo_dev:
                self._exposure_step_fused()
            return out
        # HIP renderer: the next view's preparation is enqueued before this view renders, so the
        # host reads each view's pair count while the device is still busy (no idle gap per view);
        # views rotate over NUM_STREAMS HIP streams, so one view's latency-bound binning kernels run
        # beside another's splat kernels (autograd runs each view's backward on its forward stream)
        prefetch = self.render_fn is hip_render and means.device.type == "cuda" and means.shape[0] > 0
        capture = contextlib.nullcontext()
        if self.density_stats and means.shape[0] > 0:
            if device.type == "cuda":
                self._density_check(device)
                raise ValueError(f"density_stats on {device}: this step takes the per-view autograd path, which "
                                 "collects no statistics")
            from . import cpu_renderer
            capture = cpu_renderer.capture_position_grads(self._cpu_sink(device))
        streams = [None]
        ns = min(NUM_STREAMS, len(self.my_views))
        if prefetch and ns > 1:
            main = torch.cuda.current_stream(device)
            side, _ = self._streams(device, ns)
            for st in side:
                st.wait_stream(main)  # the activations are produced on the main stream
            streams = [main] + side
        # per-stream accumulators start empty and are created by their stream's first view (a zeros
        # tensor made here on the main stream would be read by a side stream with no ordering)
        totals: list = [None for _ in streams]
        views = self.my_views

        def on(j):
            s = streams[j % len(streams)]
            return torch.cuda.stream(s) if s is not None else contextlib.nullcontext()

        # preparations run PREFETCH views ahead (each on its view's stream), so the host's wait for a
        # view's pair count is for work enqueued well before
        ahead = {}

        def prepare(j):
            if prefetch and j < len(views) and j not in ahead:
                with on(j):
                    ahead[j] = self._prepare(views[j], means, scales, colors, opacities)

        for j in range(PREFETCH):
            prepare(j)
        with capture:  # (density_stats off the HIP device: each render hooks its position gradients)
            for j, i in enumerate(views):
                prepare(j + PREFETCH)
                with on(j):
                    k = j % len(streams)
                    lv = self.view_loss(i, means, scales, colors, opacities, prepared=ahead.pop(j, None))
                    totals[k] = lv if totals[k] is None else totals[k] + lv
        for st in streams[1:]:
            streams[0].wait_stream(st)
        total = None
        for t in totals:
            if t is not None:
                total = t if total is None else total + t
        if total is None:
            # a rank with no views (world size > number of views): a zero loss that still reaches every
            # parameter, so backward() runs and the rank joins the all-reduce with zero gradients
            total = sum(p.sum() for p in self.params.values()) * 0.0
        loss = total / len(self.targets)
        if self.rank == 0:
            loss = loss + self.reg_opacity * opacities.mean() + self.reg_scale * scales.mean()
        loss.backward()
        out = self._finish_step(loss)
        if self.refine_cameras:  # autograd delivered d loss / d xi through pose_view (view_loss)
            self._camera_step_autograd()
        if self.exposure:  # ... and d loss / d E through the exposed colour
            self._exposure_step_autograd()
        return out

    def _native_exec(self) -> bool:
        """Whether this step's views go through the native executor (GR_NATIVE_EXEC)."""
        if NATIVE_EXEC == "auto":
            return self.width * self.height <= NATIVE_EXEC_MAX_PIXELS
        return str(NATIVE_EXEC) not in ("0", "False", "")

    def _views_native(self, means, scales, colors, opacities, depth: bool, sized=None, ssim: bool = False) -> torch.Tensor:
        """_views_scheduled's forms through the native executor (gr_fit_views): one C call per step; returns the sum
        of the view losses and leaves the stream accumulators in self._acc_parts.  ssim: the D-SSIM form
        (gr_fit_views_ssim)."""
        device = means.device
        m, s, c, o = (t.detach().float().contiguous() for t in (means, scales, colors, opacities))
        views = self.my_views
        if not views:
            self._acc_parts = [tuple(torch.zeros_like(t) for t in (m, s, c, o))]
            return torch.zeros((), device=device)
        ns = max(1, min(NUM_STREAMS, len(views)))
        w_sil, w_depth, g_scale, w_dssim = self._loss_terms(depth, ssim)
        key = (tuple(views), depth, F32_GRADE, w_sil > 0.0, str(device), sized is not None, ssim)
        cache = self._native_targets
        if cache is None or cache[0] != key:
            arr = (tr._native.GrFitTarget * len(views))()
            for j, i in enumerate(views):
                gv = self._step_view(i, device, depth, ssim)
                arr[j].view = gv if sized is None else tr.sized_view(gv)
                arr[j].target_depth = self.depths[i].data_ptr() if depth else None
                arr[j].target_rgb = self.targets[self._vi(i)].data_ptr()
                arr[j].target_mask = self.masks[self._vi(i)].data_ptr() if w_sil > 0.0 else None
            self._native_targets = cache = (key, arr)
        cfg = self._exec_config(device, ns, sized)
        losses_v = torch.empty(len(views), dtype=torch.float32, device=device)
        # (the executor writes the kept accumulators, accumulate = 0 first, only after the caller's stream)
        acc, ptrs = self._acc_sets("native", ns, m, s, c, o)
        L = tr._native.lib()
        head = (tr._native.executor(device.index or 0), ctypes.byref(cfg), len(views), cache[1], int(m.shape[0]),
                tr._native.ptr(m), tr._native.ptr(s), tr._native.ptr(c), tr._color_dim(c), tr._native.ptr(o),
                ctypes.c_float(w_sil), ctypes.c_float(w_depth), ctypes.c_float(g_scale))
        tail = (tr._native.ptr(losses_v), ptrs, ctypes_stream(device))
        if self.density_stats:  # the executor enqueues gr_density_stats beside each gr_reduce_sums of this call
            sp = (ctypes.c_void_p * ns)(*[b.data_ptr() for b in self._stats_bufs(ns, device)])
            tr._native.check(L.gr_executor_density_stats(head[0], sp), "gr_executor_density_stats")
        if self.refine_cameras:  # and gr_camera_grads_sums after it: view j of this call into row j
            tr._native.check(L.gr_executor_camera_grads(head[0], tr._native.ptr(self._camera_rows(len(views), device))),
                             "gr_executor_camera_grads")
        try:
            if ssim:
                tr._native.check(L.gr_fit_views_ssim(*head, ctypes.c_float(w_dssim), *tail), "gr_fit_views_ssim")
            else:
                tr._native.check(L.gr_fit_views(*head, *tail), "gr_fit_views")
        finally:
            if self.density_stats:  # (the executor is the device's: other fits use it without statistics)
                L.gr_executor_density_stats(head[0], None)
            if self.refine_cameras:
                L.gr_executor_camera_grads(head[0], None)
        self._acc_parts = acc
        self._native_keep = (m, s, c, o)  # read by the executor's streams until the caller's stream passes them
        return losses_v.sum()

    def _views_fused(self, means, scales, colors, opacities, reg_t, native: bool, sized=None) -> tuple:
        """The fused step's views through the native executor or the Python schedule: (the sum of the view losses,
        the regulariser reg_t after its hand-over).  The regulariser's small kernels follow the last preparation on
        the preparation stream (_reg_after_exec; the L1 form's tail_fn: neither before the first view nor between the
        last reduction and the parameter update); the depth and D-SSIM forms of the Python schedule take it as it is."""
        reg_fn = (lambda: reg_t) if reg_t is not None else None
        if native and not (self._expo_dev or self._wgt_dev):  # (the exposure and weighted forms have no executor entry:
            #                                                      the Python schedule)
            total = self._views_native(means, scales, colors, opacities, self._depth_grad(), sized=sized, ssim=self._ssim_form())
            return total, self._reg_after_exec(reg_fn, means.device)
        form = self._form()
        if form != "l1":
            return self._views_scheduled(means, scales, colors, opacities, form, sized=sized)[0], reg_t
        return self._views_scheduled(means, scales, colors, opacities, form, reg_fn, sized)

    def _views_direct(self, means, scales, colors, opacities, tail_fn=None, sized=None):
        """_views_scheduled's L1 form: (the sum of the view losses, tail_fn()'s value or None)."""
        return self._views_scheduled(means, scales, colors, opacities, "l1", tail_fn, sized)

    def _views_scheduled(self, means, scales, colors, opacities, form: str, tail_fn=None, sized=None) -> tuple:
        """This rank's views without autograd, on the Python schedule (_view_loop).  Per view, by form:
          l1     gr_fwd_render_l1 (the HIP forward whose epilogue evaluates the view's L1 + silhouette loss and its
                 upstream gradients, fit_multiview_stub.py:292-299) and gr_bwd_splat (the backward splat, :310), then
                 gr_gather_view (GATHER; else the view's workspaces wait for gr_reduce_views); band views (_vi), and
                 the binning on a stream of its own with GR_BIN_STREAM;
          depth  the depth term (fit_multiview_stub.py:301-305): the HIP forward in the default precision mode (f32-grade
                 W and D, the depth-gradient footprint) keeping its saved sums, then gr_bwd_fit_gather (L1 + silhouette
                 + depth loss gradients and the render backward up to the per-Gaussian sums);
          ssim   the D-SSIM form (dssim_fused): gr_bwd_fit_ssim_gather in its place, whose photometric term is
                 (1 - l) L1 + l D-SSIM; with a depth term the depth form's views, without one _ssim_view's;
          exposure  the exposure form (exposure_fused): gr_bwd_fit_exposure_gather in its place, whose photometric term
                 is taken on E_i (clamp01(out), 1), E_i read from the device tensor, and which writes row i of
                 self._expo_rows (d loss / d E); the D-SSIM form's views.
          weighted  the weighted form (weights): gr_bwd_fit_weighted_gather in its place, every L1 term times the view's
                 loss weights; the D-SSIM form's views.
        Every reduction batch of a stream adds its views' gradient w.r.t. the activated parameters into that stream's
        accumulator set (_reduce_batch, in view order: deterministic); the sets leave in self._acc_parts, to be summed
        in stream order by the caller (gr_fit_param_step or torch adds).  Returns (the sum of the view losses (device,
        0-d), tail_fn() evaluated on the preparation stream after the last preparation, or None)."""
        device = means.device
        m, s, c, o = (t.detach().float().contiguous() for t in (means, scales, colors, opacities))
        views = self.my_views
        nv = len(views)
        ns = max(1, min(NUM_STREAMS, nv))
        main = torch.cuda.current_stream(device)
        self._streams(device, ns)  # (made before the binning stream: creation order places them on the hardware queues)
        # made on the main stream before the render streams wait for it (_view_loop's rule 1): every stream's use is
        # ordered after its allocation, and main waits for every stream before they are read or freed
        losses_v = torch.empty(max(1, nv), dtype=torch.float32, device=device)
        acc, _ = self._acc_sets("direct", ns, m, s, c, o)
        stats = self._stats_bufs(ns, device) if self.density_stats else None
        if self.refine_cameras:
            self._camera_rows(nv, device)
        expo = form == "exposure"
        if expo:  # every view's d loss / d E row (gr_bwd_fit_exposure_gather writes its own; other ranks' stay zero)
            self._expo_rows = torch.zeros((len(self.targets), 12), dtype=torch.float32, device=device)
        wgt = form == "weighted"
        sums16 = ("ssim", "exposure", "weighted")  # the forms whose views without a depth term are _ssim_view's (16-pixel tiles)
        depth = form == "depth" or (form in sums16 and self._depth_grad())
        w_sil, w_depth, g_scale, w_dssim = self._loss_terms(depth, form == "ssim")
        bin_stream = None
        if form == "l1" and BIN_STREAM != "":
            if self._bin is None or self._bin.device != device:
                self._bin = torch.cuda.Stream(device, priority=int(BIN_STREAM))
            bin_stream = self._bin
            bin_stream.wait_stream(main)

        def body_l1(j, take):
            # one zone at the core cutoff and no depth channel: the loss reads neither depth nor the tail-only part
            # of W's footprint (torch_renderer.FIT_CUTOFF)
            i = self._vi(views[j])
            pv = take(j)
            rs, ws = tr.forward_l1_native(m, s, c, o, pv.gv, pv, self.targets[i], self.masks[i] if w_sil > 0.0 else None,
                                          w_sil, g_scale, losses_v[j:j + 1], bin_stream=bin_stream)
            pv = None
            tr.backward_splat_native(rs, ws)
            if GATHER:  # the view's sums; its bins, geom and workspace go back to the allocator on return
                return rs.gv, tr.gather_view_native(rs, ws)
            return rs, ws

        def body_sums(j, take):
            i = views[j]
            pv = take(j)
            _, _, _, rs = tr.forward_native(m, s, c, o, pv.gv, pv, images=False)  # the backward reads the sums
            pv = None
            # the entries take the same operands, the D-SSIM one its weight behind g_scale, the exposure one the view's
            # E (a row view of the device tensor: no host read) and its row of d loss / d E, the weighted one the view's
            # loss weights
            ssim = form == "ssim"
            gather = (tr.backward_fit_exposure_gather_native if expo
                      else tr.backward_fit_weighted_gather_native if wgt
                      else tr.backward_fit_ssim_gather_native if ssim else tr.backward_fit_gather_native)
            own = (self._expo[i], self._expo_rows[i]) if expo else (self.weights[i],) if wgt else (w_dssim,) if ssim else ()
            sums, sums3 = gather(rs, self.targets[i], self.masks[i] if w_sil > 0.0 else None, w_sil,
                                 self.depths[i] if depth else None, w_depth, g_scale, *own, losses_v[j:j + 1])
            return (rs.gv, sums, sums3) if sums3 is not None else (rs.gv, sums)

        gathered = GATHER or form != "l1"
        tail = self._view_loop(
            device, nv, self._preparer(m, s, c, o, lambda q: self._step_view(views[q], device, depth, form in sums16), nv, sized),
            body_l1 if form == "l1" else body_sums,
            lambda k, batch, js, accumulate: self._reduce_batch(m, s, c, o, batch, js, k, acc, stats, accumulate, gathered),
            tail_fn)
        if bin_stream is not None:
            main.wait_stream(bin_stream)
        # the streams' accumulators (summed in stream order by the caller: gr_fit_param_step or torch adds)
        self._acc_parts = acc[:min(ns, nv)] if nv > 0 else [tuple(torch.zeros_like(t) for t in (m, s, c, o))]
        return (losses_v[:nv].sum() if views else torch.zeros((), device=device)), tail

    def _fused_step_ok(self) -> bool:
        """The fused parameter update applies: plain Adam (torch.optim.Adam defaults: no weight decay, no
        amsgrad, not maximize), one parameter group, the stub's parameter names, float32 contiguous tensors on
        the HIP device (gr_fit_param_step reads them through raw pointers)."""
        if not FUSED_STEP or type(self.opt) is not torch.optim.Adam or len(self.opt.param_groups) != 1:
            return False
        if not all(p.dtype == torch.float32 and p.is_cuda and p.is_contiguous() for p in self.params.values()):
            return False
        g = self.opt.param_groups[0]
        if g["weight_decay"] != 0 or g["amsgrad"] or g.get("maximize", False) or isinstance(g["lr"], torch.Tensor):
            return False
        return set(self.params) in ({"means", "scales_raw", "opacities_raw", "colors_raw"},
                                    {"means", "scales_raw", "opacities_raw", "sh_raw"})

    def _fused_param_step(self, scales, opacities, loss, sized=None) -> torch.Tensor:
        """fit_multiview_stub.py:307-311 after the views: d loss / d raw parameters through the activations
        (softplus + 1e-3, sigmoid, identity) and the regulariser (rank 0), then torch.optim.Adam's update with
        its own state tensors: every parameter in one launch (world size 1; gr_fit_param_steps), or gradient assembly
        into the flat all-reduce buffer (gr_fit_param_step), the all-reduce, then gr_adam_step per parameter."""
        nat = tr._native
        L = nat.lib()
        g = self.opt.param_groups[0]
        lr, (b1, b2), eps = float(g["lr"]), g["betas"], float(g["eps"])
        parts = self._acc_parts
        self._acc_parts = None
        slot = {"means": 0, "scales_raw": 1, "colors_raw": 2, "sh_raw": 2, "opacities_raw": 3}
        act = {"means": nat.ACT_IDENTITY, "scales_raw": nat.ACT_SOFTPLUS, "colors_raw": nat.ACT_SIGMOID,
               "sh_raw": nat.ACT_IDENTITY, "opacities_raw": nat.ACT_SIGMOID}
        # mean()'s backward: the float32 weight divided by the float32 element count, as autograd computes it
        reg = {"scales_raw": float(np.float32(self.reg_scale) / np.float32(max(1, scales.numel()))),
               "opacities_raw": float(np.float32(self.reg_opacity) / np.float32(max(1, opacities.numel())))}
        names = list(self.params)
        plist = [self.params[k] for k in names]
        stream = ctypes_stream(plist[0].device)
        flat = None
        if self.world > 1:
            flat = torch.empty(sum(p.numel() for p in plist) + 1, dtype=torch.float32, device=plist[0].device)
        off = 0
        most = nat.FIT_MAX_ACC
        # every tensor's operands, stated once: each route below hands these entries to its entry point
        entries = (nat.GrParamStep * len(plist))()
        held = []  # the summed arrays (folded ones included), alive until their launch is issued
        for e, k, p in zip(entries, names, plist):
            st = self.opt.state[p]
            if not st:  # torch.optim.Adam's lazy state, same tensors and layout
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if sized is None:  # (a captured step: the graph driver advances the host counts per replay)
                st["step"] += 1
            t = float(st["step"])
            e.neg_step_size, e.bias_correction2_sqrt = -(lr / (1.0 - b1 ** t)), (1.0 - b2 ** t) ** 0.5
            a = [pp[slot[k]] for pp in parts]
            if len(a) > most:  # more streams than the kernel sums: fold the rest in stream order first
                t = a[most - 1]
                for x in a[most:]:
                    t = t + x
                a = a[:most - 1] + [t]
            held.append(a)
            e.num_accs = len(a)
            for j, x in enumerate(a):
                e.accs[j] = x.data_ptr()
            if flat is not None:
                grad = flat[off:off + p.numel()].view_as(p)
                off += p.numel()
            else:
                # the gradient tensor is kept across steps (zero_grad(set_to_none) drops p.grad each step; the
                # kernel overwrites every element, in stream order after the previous step's readers)
                kept = self._grad_keep.get(k)
                if kept is None or kept.shape != p.shape or kept.device != p.device:
                    self._grad_keep[k] = kept = torch.empty_like(p)
                grad = kept
            # p.grad is this kept tensor, overwritten in place every step (an alias, not a fresh tensor): a caller that
            # keeps a reference to p.grad across steps (logging, clipping history, EMA) must copy it
            p.grad = grad
            e.count, e.act = p.numel(), act[k]
            e.param, e.grad = p.data.data_ptr(), grad.data_ptr()
            e.exp_avg, e.exp_avg_sq = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
            e.reg = reg.get(k, 0.0) if self.rank == 0 else 0.0
        betas_eps = (ctypes.c_double(b1), ctypes.c_double(b2), ctypes.c_float(eps))

        def gradient(e, adam):  # one tensor's gradient, with adam its update too (gr_fit_param_step)
            nat.check(L.gr_fit_param_step(e.count, e.act, e.param, e.grad, e.accs, e.num_accs, ctypes.c_float(e.reg),
                                                 adam, e.exp_avg, e.exp_avg_sq, ctypes.c_float(e.neg_step_size),
                                                 ctypes.c_float(e.bias_correction2_sqrt), *betas_eps, stream),
                             "gr_fit_param_step")

        if flat is None:
            if len(plist) > nat.FIT_MAX_PARAMS:  # more tensors than one launch takes: one launch each
                if sized is not None:
                    raise RuntimeError("graph step: more parameters than one gr_fit_param_steps launch")
                for e in entries:
                    gradient(e, 1)
            elif sized is None:  # world size 1: every parameter's gradient and Adam update in one launch
                nat.check(L.gr_fit_param_steps(len(plist), entries, *betas_eps, stream), "gr_fit_param_steps")
            else:  # the step's scalars from the device table, skipped on overflow (gr_fit_param_steps_sched)
                nat.check(L.gr_fit_param_steps_sched(
                    len(plist), entries, *betas_eps, nat.ptr(sized.sched), nat.ptr(sized.step_dev),
                    nat.ptr(sized.ovf), ctypes.c_void_p(sized.flags.data_ptr()), stream), "gr_fit_param_steps_sched")
            return loss.detach()
        bounds, o0 = [], 0
        for p in plist:
            bounds.append((o0, o0 + p.numel()))
            o0 += p.numel()
        bounds[-1] = (bounds[-1][0], off + 1)  # the loss rides in the last bucket

        def assemble(b):
            gradient(entries[b], 0)
            if b == len(plist) - 1:
                flat[off:off + 1].copy_(loss.detach().reshape(1))

        def finish(b):
            e = entries[b]
            nat.check(L.gr_adam_step(e.count, e.param, e.grad, e.exp_avg, e.exp_avg_sq, ctypes.c_float(e.neg_step_size),
                                            ctypes.c_float(e.bias_correction2_sqrt), *betas_eps, stream), "gr_adam_step")

        bucketed_all_reduce([flat[a:b] for a, b in bounds], assemble, finish, self.group)
        return flat[off]

    def _finish_step(self, loss) -> torch.Tensor:
        plist = list(self.params.values())
        for p in plist:
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        if self.world > 1:
            flat = torch.cat([p.grad.reshape(-1) for p in plist] + [loss.detach().reshape(1)])
            bounds, off = [], 0
            for p in plist:
                bounds.append((off, off + p.numel()))
                off += p.numel()
            bounds[-1] = (bounds[-1][0], off + 1)
            buckets = [flat[a:b] for a, b in bounds]

            def finish(b):
                p = plist[b]
                p.grad.copy_(buckets[b][:p.numel()].view_as(p))

            bucketed_all_reduce(buckets, lambda b: None, finish, self.group)
            loss_all = flat[off]
        else:
            loss_all = loss.detach()
        self.opt.step()
        return loss_all

    # ---- the fused step as one HIP graph (GR_GRAPH) -------------------------------------------------------------
    def _graph_ok(self, device) -> bool:
        """The graph applies: the fused path with its one-launch parameter update (world size 1), the Python
        schedule without a separate binning stream, and the optimizer state made by an eager step.  Not the D-SSIM
        form: the batched and graph steps have none."""
        if self._ssim_form() or self.density_stats:  # (a replayed step that overflowed is redone: its statistics
            return False                             # would count twice, so a fit that collects them steps eagerly)
        if self.exposure or self.weights is not None:  # (the exposure and weighted forms have no batched / captured
            return False                               # schedule)
        if self.refine_cameras:  # (captured launches carry the view matrices as kernel arguments)
            return False
        mode = self._graph_mode()
        if not (mode != "0" and self.world == 1 and device.type == "cuda" and BIN_STREAM == "" and self._direct(device)
                and self.params["means"].shape[0] > 0 and self._fused_step_ok()):
            return False
        if mode in ("batch", "batchgraph") and F32_GRADE:  # (the batched L1 path runs the two-piece mode only)
            return False
        if min(NUM_STREAMS, len(self.my_views)) > tr._native.FIT_MAX_ACC or len(self.params) > tr._native.FIT_MAX_PARAMS:
            return False
        return all(bool(self.opt.state.get(p)) for p in self.params.values())

    def _graph_mode(self) -> str:
        """The effective GR_GRAPH mode of this fit (auto: batch for small views, else 0)."""
        if GRAPH_MODE == "auto":
            return "batch" if self.width * self.height <= GRAPH_AUTO_PIXELS and len(self.my_views) >= 2 else "0"
        return GRAPH_MODE

    def _graph_key(self) -> tuple:
        g = self.opt.param_groups[0]
        plist = list(self.params.values())
        return (tuple((p.data_ptr(), tuple(p.shape)) for p in plist),
                tuple((self.opt.state[p]["exp_avg"].data_ptr(), self.opt.state[p]["exp_avg_sq"].data_ptr()) for p in plist),
                float(g["lr"]), tuple(g["betas"]), float(g["eps"]), tuple(self.my_views), self._depth_grad(),
                self.w_sil, self.w_depth, self.reg_opacity, self.reg_scale, F32_GRADE, FIT_TILE, NUM_STREAMS,
                tuple(t.data_ptr() for t in self.targets), tuple(m.data_ptr() for m in (self.masks or ())),
                tuple(d.data_ptr() for d in (self.depths or ())))

    def _probe_counts(self, device) -> list:
        """Every view of this rank prepared once with host-read plans: [(pairs, slots, core pairs)] per view."""
        with torch.no_grad():
            m, s, c, o = (t.detach().float().contiguous() for t in activations(self.params))
            views = self.my_views
            pins = torch.zeros((max(1, len(views)), 3), dtype=torch.int64, pin_memory=True)
            depth = self._depth_grad()
            for j0 in range(0, len(views), tr._native.PREPARE_MAX_VIEWS):
                js = range(j0, min(len(views), j0 + tr._native.PREPARE_MAX_VIEWS))
                tr.prepare_views_native(m, s, c, o, [self._step_view(views[q], device, depth) for q in js],
                                        [pins[q] for q in js])
            torch.cuda.synchronize(device)
            return [tuple(int(x) for x in r) for r in pins[:len(views)].tolist()]

    @staticmethod
    def _caps_of(counts, old=None) -> list:
        def grow(x):
            return (int(x * GRAPH_MARGIN) + 4096 + 4095) // 4096 * 4096
        caps = []
        for j, (k, _, kc) in enumerate(counts):
            cc, ct = grow(kc), grow(k - kc)
            if old is not None:
                cc, ct = max(cc, int(old[j].num_core_pairs)), max(ct, int(old[j].num_pairs - old[j].num_core_pairs))
            caps.append(tr._native.GrPlan(cc + ct, cc + ct, cc))
        return caps

    def _graph_sched(self, device, t0: int):
        """(neg_step_size, bias_correction2_sqrt) of updates t0+1 .. t0+65536 onward from update 1, as the eager step
        computes them (same expressions, rounded to float32 as its ctypes arguments): index t = updates applied."""
        g = self.opt.param_groups[0]
        lr, (b1, b2) = float(g["lr"]), g["betas"]
        T = max(1 << 16, 2 * (t0 + 1))
        tab = np.empty((T, 2), dtype=np.float32)
        for t in range(T):
            u = float(t + 1)
            tab[t, 0] = -(lr / (1.0 - b1 ** u))
            tab[t, 1] = (1.0 - b2 ** u) ** 0.5
        return torch.from_numpy(tab.reshape(-1)).to(device), T

    def _act_ws_for(self, device) -> torch.Tensor:
        """activations_native's workspace, kept per fitter (made outside any capture: _graph_build asks first)."""
        ws = self._act_ws
        if ws is None or ws.device != device:
            self._act_ws = ws = torch.zeros(int(tr._native.lib().gr_fit_activations_ws_bytes(0)), dtype=torch.uint8,
                                            device=device)
        return ws

    def _activations_fused(self, device):
        """The fused step's activations and (rank 0) regulariser in one launch (activations_native)."""
        ws = self._act_ws_for(device)
        if self.params["means"].shape[0] == 0:
            means, scales, colors, opacities = activations(self.params)
            return means, scales, colors, opacities, None
        return activations_native(self.params, (self.reg_opacity, self.reg_scale) if self.rank == 0 else None, ws)

    def _graph_body(self, gs):
        """The fused step (step()'s first branch, eager) on device-sized views, for capture."""
        with torch.no_grad():
            means, scales, colors, opacities, reg_t = self._activations_fused(self.params["means"].device)
            mode = self._graph_mode()
            if mode in ("batch", "batchgraph"):  # one launch per kernel for up to 8 views (gr_fit_views_batched), one stream
                total, reg = self._views_batched(means, scales, colors, opacities, gs), reg_t
            else:  # "exec": the native executor with capacities; else the Python schedule (as step()'s fused branch)
                total, reg = self._views_fused(means, scales, colors, opacities, reg_t, mode == "exec", sized=gs)
            loss = total / len(self.targets)
            if reg is not None:
                loss = loss + reg
        return self._fused_param_step(scales, opacities, loss, sized=gs)

    def _graph_build(self, device, counts=None, old_caps=None):
        """(Re)capture the step: capacities from `counts` (or a probe), the device step counter at the updates applied
        so far (the optimizer's step count), a fresh schedule table when it runs short."""
        gs = self._gs
        if gs is None:
            gs = self._gs = _GraphState()
        gs.graph = None
        n_views = max(1, len(self.my_views))
        t0 = int(float(self.opt.state[next(iter(self.params.values()))]["step"]))
        if counts is None:
            counts = self._probe_counts(device)
        gs.caps = self._caps_of(counts, old_caps)
        gs.caps_arr = (tr._native.GrPlan * max(1, len(gs.caps)))(*gs.caps)
        gs.observed = torch.zeros((n_views, 3), dtype=torch.int64, pin_memory=True)
        gs.flags = torch.zeros(2, dtype=torch.int32, pin_memory=True)
        gs.ovf = torch.zeros(1, dtype=torch.int32, device=device)
        gs.step_dev = torch.tensor([t0], dtype=torch.int32, device=device)
        if gs.sched is None or gs.sched_len < t0 + 1024 or gs.sched_key != self._graph_key()[2:5]:
            gs.sched, gs.sched_len = self._graph_sched(device, t0)
            gs.sched_key = self._graph_key()[2:5]
        gs.done_host = t0
        self._act_ws_for(device)  # (made before any capture)
        torch.cuda.synchronize(device)
        if self._graph_mode() in ("1", "batchgraph"):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="relaxed"):
                gs.loss = self._graph_body(gs)
        else:  # (diagnostics: the device-sized step without the graph, enqueued by the host every step)
            g = _EagerReplay(lambda: self._graph_body(gs), gs)
        gs.graph = g
        gs.builds += 1
        gs.key = self._graph_key()
        gs.n = int(self.params["means"].shape[0])
        gs.inflight = []
        return gs

    def _graph_step(self, device) -> torch.Tensor:
        gs = self._gs
        if gs is None or gs.graph is None or gs.key != self._graph_key():
            self.graph_sync()
            counts = None
            if gs is not None and gs.graph is not None and gs.n == int(self.params["means"].shape[0]):
                counts = [tuple(int(x) for x in r) for r in gs.observed[:len(self.my_views)].tolist()]
            gs = self._graph_build(device, counts)
        elif int(float(self.opt.state[next(iter(self.params.values()))]["step"])) + 2 >= gs.sched_len:
            self.graph_sync()
            gs = self._graph_build(device, [tuple(int(x) for x in r) for r in gs.observed[:len(self.my_views)].tolist()],
                                   gs.caps)
        gs.graph.replay()
        out = gs.loss.detach().clone()
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        for p in self.params.values():  # torch.optim.Adam's host step count, as the eager step advances it
            self.opt.state[p]["step"] += 1
        gs.inflight.append((out, ev))
        if len(gs.inflight) > 2:
            gs.inflight.pop(0)
        if len(gs.inflight) == 2:  # the previous step (the GPU is busy with this one meanwhile)
            gs.inflight[0][1].synchronize()
            self._graph_check(device)
        return out

    def _graph_check(self, device) -> None:
        """A replayed step whose views exceeded their capacities updated nothing (and neither did any later one: the
        parameters did not change): grow the capacities from the true counts, recapture, and redo those steps, their
        losses written into the tensors step() returned for them."""
        gs = self._gs
        while int(gs.flags[0]) != 0:
            torch.cuda.synchronize(device)
            done = int(gs.flags[1])
            applied = int(float(self.opt.state[next(iter(self.params.values()))]["step"]))
            lost = applied - done
            redo = gs.inflight[len(gs.inflight) - lost:] if lost > 0 else []
            counts = [tuple(int(x) for x in r) for r in gs.observed[:len(self.my_views)].tolist()]
            for p in self.params.values():
                self.opt.state[p]["step"] -= lost
            gs.overflows += 1
            inflight = gs.inflight
            gs = self._graph_build(device, counts, gs.caps)
            for out, _ in redo:  # (an overflowing redo updates nothing, nor do the ones after it: counted next round)
                gs.graph.replay()
                out.copy_(gs.loss)
                for p in self.params.values():
                    self.opt.state[p]["step"] += 1
            torch.cuda.synchronize(device)
            gs.inflight = inflight

    def _views_batched(self, means, scales, colors, opacities, gs) -> torch.Tensor:
        """The step's views on the current stream, every kernel launched once per batch of up to 8 views
        (gr_fit_views_batched) on device-sized views: the preparations (gr_fwd_prepare_views_sized, 4 views each), the
        batched chain (binning, forward with the loss epilogue or the depth-loss forward, backward, gather), then the
        chain rules of up to 16 views per gr_reduce_sums into one accumulator set.  Per-view workspaces sized by the
        capacities are kept in the graph state across steps."""
        device = means.device
        L = tr._native.lib()
        nat = tr._native
        m, s, c, o = (t.detach().float().contiguous() for t in (means, scales, colors, opacities))
        n = int(m.shape[0])
        views = self.my_views
        depth = self._depth_grad()
        w_sil, w_depth, g_scale, _ = self._loss_terms(depth)
        bkey = (n, depth, tuple((int(cp.num_pairs), int(cp.num_core_pairs)) for cp in gs.caps), str(device))
        bw = getattr(gs, "batch_ws", None)
        if bw is None or bw[0] != bkey:
            gvs = [tr.sized_view(self._step_view(i, device, depth)) for i in views]
            u8 = dict(dtype=torch.uint8, device=device)
            gb = int(L.gr_geom_bytes(n))
            ws = []
            for j, gv in enumerate(gvs):
                cp = gs.caps[j]
                ws.append(dict(
                    geom=torch.empty((gb,), **u8),
                    bins=torch.empty((int(L.gr_bins_bytes(ctypes.byref(gv), n, ctypes.byref(cp))),), **u8),
                    scratch=torch.empty((int(L.gr_fwd_scratch_bytes(ctypes.byref(gv), n, ctypes.byref(cp))),), **u8),
                    ws=torch.empty((int(L.gr_bwd_bytes(ctypes.byref(gv), n, ctypes.byref(cp))),), **u8),
                    saved=(torch.empty((int(L.gr_saved_floats(ctypes.byref(gv))),), dtype=torch.float32, device=device)
                           if depth else None),
                    sums=torch.empty((n, 8), dtype=torch.float32, device=device),
                    sums3=torch.empty((n,), dtype=torch.float32, device=device) if depth else None))
            gs.batch_ws = bw = (bkey, gvs, ws)
        _, gvs, ws = bw
        losses_v = torch.empty(max(1, len(views)), dtype=torch.float32, device=device)
        # the chain rules in one accumulator set, batches of up to REDUCE_BATCH views (every view is gathered before
        # the first chain rule, so no short tail batch): the same sums in the same order as _views_scheduled with
        # GR_STREAMS=1 and GR_REDUCE_TAIL=0, so the same parameters bit for bit (one chain-rule
        # launch for up to 16 views, one accumulator for the update to read instead of one per stream)
        ns = 1
        acc, _ = self._acc_sets("direct", ns, m, s, c, o)
        stream = ctypes_stream(device)
        cd = tr._color_dim(c)
        for j0 in range(0, len(views), nat.PREPARE_MAX_VIEWS):
            js = range(j0, min(len(views), j0 + nat.PREPARE_MAX_VIEWS))
            k = len(js)
            nat.check(L.gr_fwd_prepare_views_sized(
                k, (nat.GrView * k)(*[gvs[q] for q in js]), n, nat.ptr(m), nat.ptr(s), nat.ptr(c), cd, nat.ptr(o),
                (ctypes.c_void_p * k)(*[ws[q]["geom"].data_ptr() for q in js]), ws[js[0]]["geom"].numel(),
                (nat.GrPlan * k)(*[gs.caps[q] for q in js]),
                (ctypes.c_void_p * k)(*[gs.observed[q].data_ptr() for q in js]), nat.ptr(gs.ovf), stream),
                "gr_fwd_prepare_views_sized")
        for j0 in range(0, len(views), nat.BATCH_MAX_VIEWS):
            js = range(j0, min(len(views), j0 + nat.BATCH_MAX_VIEWS))
            arr = (nat.GrBatchView * len(js))()
            for e, q in zip(arr, js):
                w, i = ws[q], views[q]
                e.view, e.plan = gvs[q], gs.caps[q]
                e.geom, e.bins, e.bins_bytes = w["geom"].data_ptr(), w["bins"].data_ptr(), w["bins"].numel()
                e.scratch, e.scratch_bytes = w["scratch"].data_ptr(), w["scratch"].numel()
                e.ws, e.ws_bytes = w["ws"].data_ptr(), w["ws"].numel()
                e.saved = w["saved"].data_ptr() if depth else None
                e.target_rgb = self.targets[self._vi(i)].data_ptr()
                e.target_mask = self.masks[self._vi(i)].data_ptr() if w_sil > 0.0 else None
                e.target_depth = self.depths[i].data_ptr() if depth else None
                e.sums, e.sums3 = w["sums"].data_ptr(), (w["sums3"].data_ptr() if depth else None)
                e.loss = losses_v[q:q + 1].data_ptr()
            nat.check(L.gr_fit_views_batched(len(js), arr, n, ctypes.c_float(w_sil), ctypes.c_float(w_depth),
                                             ctypes.c_float(g_scale), stream), "gr_fit_views_batched")
        for k, sizes in enumerate(_batch_sizes(ns, len(views), tail=0)):
            mine = list(range(k, len(views), ns))
            at = 0
            for b in sizes:
                js = mine[at:at + b]
                if js:
                    tr.reduce_sums_native(m, s, c, o,
                                          [(gvs[q], ws[q]["sums"]) + ((ws[q]["sums3"],) if depth else ()) for q in js],
                                          acc[k], accumulate=at > 0)
                at += b
        self._acc_parts = acc[:min(ns, len(views))] if views else [tuple(torch.zeros_like(t) for t in (m, s, c, o))]
        self._native_keep = (m, s, c, o)
        return losses_v[:len(views)].sum() if views else torch.zeros((), device=device)

    def _graph_leave(self) -> None:
        """The step goes eager while replayed steps may still be in flight (the graph's conditions changed, e.g.
        F32_GRADE toggled): settle them first (an overflowed one is redone and its loss rewritten, and the host's Adam
        step count corrected), then drop the graph, so that a later capture counts only its own replays."""
        gs = self._gs
        if gs is None or gs.graph is None:
            return
        self.graph_sync()
        gs.graph = None
        gs.key = None
        gs.inflight = []

    def graph_sync(self) -> None:
        """Wait for the replayed steps and redo any that overflowed (densify, the parameters' readers and the end of a
        fit call this; a no-op without a graph)."""
        gs = self._gs
        if gs is None or gs.graph is None:
            return
        torch.cuda.synchronize(self.params["means"].device)
        self._graph_check(self.params["means"].device)

    # ---- evaluation (held-out view metrics) ---------------------------------------------------------------------
    def _eval_view(self, cam, device) -> "tr._native.GrView":
        """The gr_view an evaluation renders ``cam`` with (_gr_view's `eval`)."""
        return self._gr_view("eval", cam, device)

    def _eval_native_ok(self, device, targets) -> bool:
        """evaluate() through the HIP metrics kernel: the preconditions of _direct() that concern it (the HIP render
        op, float32 parameters, targets of exactly the image's shape read through raw pointers)."""
        shape = (self.height, self.width, 3)
        return (self.render_fn is hip_render and device.type == "cuda"
                and all(p.dtype == torch.float32 for p in self.params.values())
                and all(isinstance(t, torch.Tensor) and tuple(t.shape) == shape and t.dtype == torch.float32
                        and t.is_contiguous() and t.device == device for t in targets))

    def _eval_activations(self, device):
        """The step's own activations (gr_fit_activations where the fused step forms them, else activations())."""
        if (device.type == "cuda" and self.params["means"].shape[0] > 0 and self._fused_step_ok()):
            return activations_native(self.params)[:4]
        return tuple(t.detach() for t in activations(self.params))

    def _exec_views(self, fn: str, m, s, c, o, gvs, targets, out, extra: tuple = (), masks=None) -> None:
        """One native executor call over views that are only rendered: gr_eval_views (the views' metrics against
        ``targets`` into ``out`` (len(gvs), 3)), gr_eval_views_cc (the same with the corrected metrics and the transform:
        ``out`` (len(gvs), 18), ``extra`` its ridge, the argument before ``out``), gr_contrib_views (targets None: every
        view's peak blend weights into the one ``out``) or gr_error_views (every view's blend-weighted error against
        ``targets`` into the one ``out``).  ``extra``: the entry's own arguments before ``out``.  gr_eval_views_masked:
        ``masks`` the views' (H, W) masks, ``out`` (len(gvs), 9): the 3 metrics and the 6 masked ones."""
        device = m.device
        arr = (tr._native.GrFitTarget * len(gvs))()
        for j, gv in enumerate(gvs):
            arr[j].view = gv
            arr[j].target_rgb = targets[j].data_ptr() if targets is not None else None
            arr[j].target_mask = masks[j].data_ptr() if masks is not None else None
            arr[j].target_depth = None
        cfg = self._exec_config(device, max(1, min(NUM_STREAMS, len(gvs))))
        tr._native.check(getattr(tr._native.lib(), fn)(
            tr._native.executor(device.index or 0), ctypes.byref(cfg), len(gvs), arr, int(m.shape[0]), tr._native.ptr(m),
            tr._native.ptr(s), tr._native.ptr(c), tr._color_dim(c), tr._native.ptr(o), *extra, tr._native.ptr(out),
            ctypes_stream(device)), fn)
        self._eval_keep = (m, s, c, o)  # read by the executor's streams until the caller's stream passes them

    def _pass_direct(self, m, s, c, o, gvs, view_call: Callable) -> None:
        """The Python schedule of a render-only executor pass's calls (_view_loop): per view forward_native (saved sums
        only) + ``view_call(j, rs, pv)``, the pass's one native call on view j's render state and Prepared."""
        def body(j, take):
            pv = take(j)
            _, _, _, rs = tr.forward_native(m, s, c, o, pv.gv, pv, images=False)
            view_call(j, rs, pv)

        self._view_loop(m.device, len(gvs), self._preparer(m, s, c, o, gvs.__getitem__, len(gvs)), body)

    def _pass_views(self, fn: str, m, s, c, o, gvs, targets, out, view_call: Callable, extra: tuple = (), masks=None) -> None:
        """A render-only pass over ``gvs``: the native executor's ``fn`` (_exec_views, ``extra`` its own arguments, ``masks``
        the views' masks where it reads them) where the fit step uses it, else the Python schedule of the same calls
        (_pass_direct)."""
        if self._native_exec() and GATHER:
            self._exec_views(fn, m, s, c, o, gvs, targets, out, extra, masks)
        else:
            self._pass_direct(m, s, c, o, gvs, view_call)

    def evaluate(self, cams: Optional[list] = None, targets: Optional[list] = None, color_correct: bool = False,
                 ridge: float = losses.CC_RIDGE, masks=None) -> dict:
        """Per-view metrics of the current Gaussians against target images: float64 numpy arrays ``l1`` (mean|x - y|),
        ``mse``, ``psnr`` (-10 log10 mse, formed on the host in double; inf at zero error) and ``ssim`` in the order of
        the views passed, and their means ``mean_l1`` .. ``mean_ssim``.  Default views: the fitter's own training
        views; held-out ones are passed as ``cams`` and ``targets`` ((H, W, 3) images).  The rendered image is the one
        render_gaussians_torch(..., depth_grad=False) gives for the saved Gaussians with the fitter's background
        (16-pixel tiles, the 7-sigma footprint: the image a user will render, not the fit path's footprint).
        A collective: view i belongs to rank i % world, the results meet in one all-reduce of a zero-filled (V, 3)
        tensor (one non-zero contributor per entry: exact), every rank returns the same dict.
        On the HIP device (the HIP render op, float32 parameters and exact-shape float32 targets) the metrics come from
        the saved sums without an image (gr_eval_view), through the native executor (gr_eval_views) where the fit step
        uses it, else a Python schedule of the same calls; otherwise render_fn under no_grad and
        losses.image_metrics.  Changes nothing of the fit: no gradient, optimizer, density or random state.
        color_correct=True: the dict gains ``cc_l1``, ``cc_mse``, ``cc_psnr``, ``cc_ssim`` and their ``mean_cc_*``, the
        same metrics of each view's render mapped onto its target by the view's best affine colour transform (fitted in
        closed form with ``ridge`` towards the identity, include/gr_hip.h: a reading that a per-view exposure or white
        balance of the photos does not move, for training and held-out views alike), and ``cc_transform``, the (V, 3, 4)
        float64 array of those transforms.  On the HIP device gr_eval_views_cc (else the Python schedule of
        gr_eval_view, gr_cc_fit_view, gr_eval_view_cc), otherwise losses.image_metrics_cc; the all-reduced tensor is
        (V, 18).  With False the call, the dict and its bits are as without the argument.
        masks: a list of (H, W) masks, one per evaluated view (values as weights, expected in [0, 1]), or True for the
        fitter's own training masks (the default views only).  The dict gains ``fg_fraction`` (the mask's mean),
        ``fg_l1``, ``fg_mse``, ``fg_psnr``, ``fg_ssim`` (the metrics weighted by the mask, over its sum: the object, not
        the background; NaN for a view whose mask is empty), ``sil_l1`` (mean|alpha - mask|, the fit's silhouette term
        unweighted) and ``sil_iou`` (alpha and mask thresholded at 0.5), include/gr_hip.h, and their ``mean_*``: the
        ``mean_fg_*`` over the views with a non-empty mask (NaN if there is none), the ``mean_sil_*`` over all views.  On
        the HIP device, with exact-shape float32 contiguous masks there, gr_eval_views_masked (else the Python schedule
        of gr_eval_view and gr_eval_view_masked, one render serving both); otherwise render_fn's image and alpha and
        losses.image_metrics_masked.  Six more columns of the one all-reduced tensor.  With color_correct=True the two
        passes run one after the other, each with its own render.  The plain keys keep their bits; None: as without
        the argument."""
        self.graph_sync()
        if color_correct and not (math.isfinite(ridge) and ridge > 0.0):
            raise ValueError(f"evaluate: ridge must be positive and finite, got {ridge}")
        if (cams is None) != (targets is None):
            raise ValueError("evaluate: pass both cams and targets, or neither (the training views)")
        if cams is None:
            cams, targets = self.cams, self.targets
        if len(cams) != len(targets):
            raise ValueError(f"evaluate: {len(cams)} cameras for {len(targets)} targets")
        if masks is True:
            if cams is not self.cams:
                raise ValueError("evaluate: masks=True means the training views' masks; pass the masks of other views")
            if self.masks is None:
                raise ValueError("evaluate: masks=True, but the fitter has no masks")
            masks = self.masks
        if masks is not None:
            if not isinstance(masks, (list, tuple)) or len(masks) != len(targets):
                raise ValueError(f"evaluate: masks is a list of one (H, W) mask per view ({len(targets)}), or True")
            for k in masks:
                if not isinstance(k, torch.Tensor) or tuple(k.shape) != (self.height, self.width):
                    raise ValueError(f"evaluate: a mask is a ({self.height}, {self.width}) tensor, got "
                                     f"{tuple(k.shape) if isinstance(k, torch.Tensor) else type(k)}")
        V = len(targets)
        device = self.params["means"].device
        n = int(self.params["means"].shape[0])
        mine = list(range(self.rank, V, self.world))
        NM = tr._native.EVAL_METRICS
        cols = tr._native.EVAL_CC_ROW if color_correct else NM
        NK = tr._native.EVAL_MASK_METRICS if masks is not None else 0  # the masked metrics: the row's last columns
        res = torch.zeros((V, cols + NK), dtype=torch.float32, device=device)
        with torch.no_grad():
            means, scales, colors, opacities = self._eval_activations(device)
            if (mine and n > 0 and self._eval_native_ok(device, [targets[i] for i in mine])
                    and (masks is None or all(k.dtype == torch.float32 and k.is_contiguous() and k.device == device
                                              for k in (masks[i] for i in mine)))):
                m, s, c, o = (t.detach().float().contiguous() for t in (means, scales, colors, opacities))
                gvs = [self._eval_view(cams[i], device) for i in mine]
                tg = [targets[i] for i in mine]
                if color_correct or masks is None:
                    out = torch.empty((len(mine), cols), dtype=torch.float32, device=device)
                    if color_correct:
                        def view_cc(j, rs, pv):  # the executor's three calls on the view's saved sums, into its row
                            tr.eval_view_native(rs, tg[j], out[j, :NM])
                            tr.cc_fit_view_native(rs, tg[j], out[j, 2 * NM:], ridge)
                            tr.eval_view_cc_native(rs, tg[j], out[j, 2 * NM:], out[j, NM:2 * NM])

                        self._pass_views("gr_eval_views_cc", m, s, c, o, gvs, tg, out, view_cc, (ctypes.c_float(ridge),))
                    else:
                        self._pass_views("gr_eval_views", m, s, c, o, gvs, tg, out,
                                         lambda j, rs, pv: tr.eval_view_native(rs, tg[j], out[j]))
                    res[mine, :cols] = out
                if masks is not None:  # (beside color_correct: a pass of its own, with its own render)
                    mk = [masks[i] for i in mine]
                    outm = torch.empty((len(mine), NM + NK), dtype=torch.float32, device=device)

                    def view_masked(j, rs, pv):  # the executor's two calls on the view's saved sums, into its row
                        tr.eval_view_native(rs, tg[j], outm[j, :NM])
                        tr.eval_view_masked_native(rs, tg[j], mk[j], outm[j, NM:])

                    self._pass_views("gr_eval_views_masked", m, s, c, o, gvs, tg, outm, view_masked, masks=mk)
                    if not color_correct:
                        res[mine, :NM] = outm[:, :NM]
                    res[mine, cols:] = outm[:, NM:]
            else:
                for i in mine:
                    kw = {"depth_grad": False} if self.render_fn is hip_render else {}
                    pred = self.render_fn(means, scales, colors, opacities, cams[i], self.width, self.height,
                                          self._background(device), **kw)
                    if masks is not None:
                        if not (isinstance(pred, tuple) and len(pred) >= 2):
                            raise ValueError("evaluate: masks need a render_fn that returns the alpha beside the image")
                        mm = losses.image_metrics_masked(pred[0], pred[1], targets[i].to(device), masks[i].to(device))
                        res[i, cols:] = torch.stack([torch.nan_to_num(mm[k], nan=0.0) for k in MASK_KEYS]).to(res)
                    pred = pred[0] if isinstance(pred, tuple) else pred
                    if color_correct:
                        mt = losses.image_metrics_cc(pred, targets[i].to(device), ridge)
                        res[i, :cols] = torch.cat([torch.stack([mt[p + k] for p in ("", "cc_") for k in ("l1", "mse", "ssim")]),
                                                   mt["cc_transform"].reshape(-1)]).to(res)
                    else:
                        mt = losses.image_metrics(pred, targets[i].to(device))
                        res[i, :cols] = torch.stack([mt["l1"], mt["mse"], mt["ssim"]]).to(res)
        if self.world > 1:
            dist.all_reduce(res, group=self.group)
        a = res.double().cpu().numpy()
        l1, mse, ssim = a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()
        with np.errstate(divide="ignore"):
            psnr = -10.0 * np.log10(mse)
        mean = lambda x: float(x.mean()) if V else float("nan")  # noqa: E731
        r = {"l1": l1, "mse": mse, "psnr": psnr, "ssim": ssim, "mean_l1": mean(l1), "mean_mse": mean(mse),
             "mean_psnr": mean(psnr), "mean_ssim": mean(ssim)}
        if color_correct:
            cl1, cmse, cssim = a[:, NM].copy(), a[:, NM + 1].copy(), a[:, NM + 2].copy()
            with np.errstate(divide="ignore"):
                cpsnr = -10.0 * np.log10(cmse)
            r.update({"cc_l1": cl1, "cc_mse": cmse, "cc_psnr": cpsnr, "cc_ssim": cssim, "mean_cc_l1": mean(cl1),
                      "mean_cc_mse": mean(cmse), "mean_cc_psnr": mean(cpsnr), "mean_cc_ssim": mean(cssim),
                      "cc_transform": a[:, 2 * NM:2 * NM + tr._native.CC_TRANSFORM].reshape(V, 3, 4).copy()})
        if masks is not None:
            k = {name: a[:, cols + q].copy() for q, name in enumerate(MASK_KEYS)}
            some = k["fg_fraction"] > 0.0  # (an empty mask: the row holds zeros there)
            for name in ("fg_l1", "fg_mse", "fg_ssim"):
                k[name][~some] = np.nan
            with np.errstate(divide="ignore"):
                k["fg_psnr"] = -10.0 * np.log10(k["fg_mse"])
            for name in ("fg_fraction", "fg_l1", "fg_mse", "fg_psnr", "fg_ssim", "sil_l1", "sil_iou"):
                r[name] = k[name]
                over = k[name][some] if name.startswith("fg_") and name != "fg_fraction" else k[name]
                r["mean_" + name] = float(over.mean()) if len(over) else float("nan")
        return r

    # ---- contribution (peak blend weight per Gaussian) ----------------------------------------------------------
    def contribution_state(self, cams: Optional[list] = None) -> torch.Tensor:
        """Per Gaussian in canonical order (as canonical_params), its peak blend weight: the maximum over the views
        ``cams`` (default: the training cameras) and their pixels of w / (1 + W), its share of the pixel under this
        renderer's weighted-average compositing.  Removing Gaussian i alone moves no pixel of those views by more than
        peak[i] / (1 - peak[i]) in any channel.  (N,) float32 on the parameters' device.
        The views are rendered as evaluate() renders them (16-pixel tiles, the 7-sigma footprint, the step's own
        activations).  A collective: view i belongs to rank i % world, the ranks meet in one all-reduce (MAX: exact),
        every rank returns the same tensor.  On the HIP device through gr_contrib_view (the native executor's
        gr_contrib_views where the fit step uses it, else a Python schedule of the same calls); on other devices
        cpu_renderer.peak_contribution.  Changes nothing of the fit."""
        self.graph_sync()
        cams = self.cams if cams is None else cams

        def cpu_view(i, m, s, c, o):
            from . import cpu_renderer
            return cpu_renderer.peak_contribution(m, s, o, cams[i].view, cams[i].proj, self.width, self.height)

        return self._gaussian_state(cams, None, "gr_contrib_views",
                                    lambda rs, pv, _target, peak: tr.contrib_view_native(rs, pv, peak), cpu_view)

    def _gaussian_state(self, cams, targets, fn: str, view_call: Callable, cpu_view: Callable,
                        unmet: Optional[str] = None) -> torch.Tensor:
        """contribution_state's and error_state's flow: this rank's share of ``cams`` (rendered against ``targets``, or
        None), every view's values folded by maximum into one zeroed (n,) buffer, all-reduced (MAX) and scattered to
        canonical order.  On the HIP device the render-only pass ``fn`` (_pass_views; per view
        ``view_call(rs, pv, target, out)``), with targets only under _eval_native_ok (else ValueError(``unmet``)); on
        other devices ``cpu_view(i, m, s, c, o)`` per view."""
        device = self.params["means"].device
        n = int(self.params["means"].shape[0])
        mine = list(range(self.rank, len(cams), self.world))
        stat = torch.zeros((n,), dtype=torch.float32, device=device)
        with torch.no_grad():
            if mine and n > 0:
                m, s, c, o = (t.detach().float().contiguous() for t in self._eval_activations(device))
                if device.type == "cuda":
                    tg = None if targets is None else [targets[i] for i in mine]
                    if tg is not None and not self._eval_native_ok(device, tg):
                        raise ValueError(unmet)
                    gvs = [self._eval_view(cams[i], device) for i in mine]
                    self._pass_views(fn, m, s, c, o, gvs, tg, stat,
                                     lambda j, rs, pv: view_call(rs, pv, None if tg is None else tg[j], stat))
                else:
                    for i in mine:
                        stat = torch.maximum(stat, cpu_view(i, m, s, c, o))
        if self.world > 1:
            dist.all_reduce(stat, op=dist.ReduceOp.MAX, group=self.group)
        if self.perm is not None:
            canon = torch.empty_like(stat)
            canon[self.perm] = stat
            stat = canon
        return stat

    # ---- error (blend-weighted pixel error per Gaussian) --------------------------------------------------------
    def error_state(self, cams: Optional[list] = None, targets: Optional[list] = None) -> torch.Tensor:
        """Per Gaussian in canonical order (as canonical_params), its blend-weighted pixel error: the maximum over the
        views (default: the training views; else ``cams`` and ``targets``, (H, W, 3) images, both or neither) of
        sum_p b_i(p) e(p), b = w / (1 + W) the Gaussian's blend weight and e the mean absolute colour error of the
        pixel.  The blend weights and the background's 1 / (1 + W) sum to one, so per view the values and the
        background's share add up to the view's summed L1 error: the unit is pixels x colour error.  (N,) float32 on
        the parameters' device.
        The views are rendered as evaluate() renders them.  A collective: view i belongs to rank i % world, the ranks
        meet in one all-reduce (MAX: exact), every rank returns the same tensor.  On the HIP device through
        gr_error_view (the native executor's gr_error_views where the fit step uses it, else a Python schedule of the
        same calls), under evaluate()'s conditions for its HIP kernel (it raises when they do not hold: there is no
        other form on that device); on other devices cpu_renderer.blend_error, which with exposure=True and the
        default views compares E_v (x, 1) with the target as the fit's photometric term does (caller-passed cameras
        have no exposure).  Collected on demand, nothing during steps.  Changes nothing of the fit."""
        self.graph_sync()
        if (cams is None) != (targets is None):
            raise ValueError("error_state: pass both cams and targets, or neither (the training views)")
        own = cams is None
        if own:
            cams, targets = self.cams, self.targets
        if len(cams) != len(targets):
            raise ValueError(f"error_state: {len(cams)} cameras for {len(targets)} targets")
        device = self.params["means"].device

        def cpu_view(i, m, s, c, o):
            from . import cpu_renderer
            E = self._expo.detach() if (own and self.exposure) else None
            return cpu_renderer.blend_error(m, s, c, o, cams[i].view, cams[i].proj, self.width, self.height, targets[i],
                                            self._background(device), exposure=None if E is None else E[i])

        return self._gaussian_state(
            cams, targets, "gr_error_views", tr.error_view_native, cpu_view,
            unmet="error_state on the HIP device needs the HIP render op, float32 parameters and "
                  f"contiguous float32 targets of shape {(self.height, self.width, 3)} on {device}: "
                  "gr_error_view reads them through raw pointers and has no other form")

    def densify_and_prune(self, max_gaussians: int, densify_ratio: float, prune_opacity: float,
                          on_device: Optional[bool] = None, mode: str = "opacity", grad_threshold: float = 0.0002,
                          split_scale: float = 0.01, prune_mode: str = "opacity",
                          prune_contribution: float = 1.0 / 510.0, error_threshold: float = 0.0) -> None:
        """on_device (default: N >= DEVICE_DENSIFY_MIN): the device-side rule with a device generator
        (densify_and_prune_device); otherwise the host rule with the stub's CPU random stream.
        mode "gradient" (a fitter with density_stats): densify_by_gradient on the statistics since the last call, on
        the parameters' device with its generator (densify_ratio <= 0: prune only); the same rank-0-decides flow.
        Either mode leaves the statistics zeroed at the new size.
        mode "error" (any fitter: no density_stats, nothing collected during steps): densify_by_error on error_state(),
        taken here once, on the parameters' device with its generator: the kept Gaussians with err > error_threshold,
        the largest first, at most int(kept * densify_ratio) of them (densify_ratio <= 0: prune only).  Fills
        self.error_report (n, p50 / p90 / p99 / max of err, the count over the threshold; the clones and splits made
        on the rank that decides, rank 0).
        prune_mode "contribution": the rows that survive are prune_by_contribution(contribution_state(),
        prune_contribution) instead of the opacity rule's (whichever densify mode is active; prune_opacity is then only
        counted for the report).  The default threshold 1 / 510 bounds the change of any training pixel by half an
        8-bit level (t / (1 - t) = 1 / 509) per removed Gaussian.  Fills self.contribution_report."""
        if mode not in ("opacity", "gradient", "error"):
            raise ValueError(f"densify mode must be 'opacity', 'gradient' or 'error', got {mode!r}")
        if prune_mode not in ("opacity", "contribution"):
            raise ValueError(f"prune mode must be 'opacity' or 'contribution', got {prune_mode!r}")
        self.graph_sync()
        state = self.density_state() if mode == "gradient" else None  # (a collective: before rank 0 decides)
        err = self.error_state() if mode == "error" else None  # (a collective too)
        n_now = int(self.params["means"].shape[0])
        keep = None
        if prune_mode == "contribution":
            peak = self.contribution_state()  # (a collective too)
            keep = prune_by_contribution(peak, prune_contribution)
            pk = peak.float().cpu()
            qs = torch.quantile(pk, torch.tensor([0.01, 0.1, 0.5])).tolist() if pk.numel() else [0.0] * 3
            op_c = torch.empty_like(self.params["opacities_raw"].detach())
            if self.perm is not None:
                op_c[self.perm] = self.params["opacities_raw"].detach()
            else:
                op_c.copy_(self.params["opacities_raw"].detach())
            by_op = torch.sigmoid(op_c) <= prune_opacity
            self.contribution_report = {"n": n_now, "p1": qs[0], "p10": qs[1], "p50": qs[2],
                                        "threshold": float(prune_contribution),
                                        "at_or_below": int((peak <= prune_contribution).sum()),
                                        "pruned": int((~keep).sum()), "opacity_would_prune": int(by_op.sum()),
                                        "both": int((by_op & ~keep.to(by_op.device)).sum())}
        if mode == "gradient":
            on_device = True
            # what the threshold is compared with, for the caller's log: percentiles of avg over the seen Gaussians
            avg = (state[0] / state[1].clamp_min(1.0))[state[1] > 0].float().cpu()
            qs = torch.quantile(avg, torch.tensor([0.5, 0.9, 0.99])).tolist() if avg.numel() else [0.0] * 3
            self.density_report = {"seen": int(avg.numel()), "n": n_now, "p50": qs[0], "p90": qs[1], "p99": qs[2],
                                   "max": float(avg.max()) if avg.numel() else 0.0,
                                   "over": int((avg >= grad_threshold).sum())}
        if mode == "error":
            on_device = True
            ec = err.float().cpu()
            qs = torch.quantile(ec, torch.tensor([0.5, 0.9, 0.99])).tolist() if ec.numel() else [0.0] * 3
            self.error_report = {"n": n_now, "p50": qs[0], "p90": qs[1], "p99": qs[2],
                                 "max": float(ec.max()) if ec.numel() else 0.0, "threshold": float(error_threshold),
                                 "over": int((ec > error_threshold).sum()), "clones": 0, "splits": 0}
        if on_device is None:
            on_device = self.params["means"].device.type == "cuda" and n_now >= DEVICE_DENSIFY_MIN
        if on_device and self._dgen is None:
            self._dgen = torch.Generator(device=self.params["means"].device).manual_seed(self.densify_seed)

        def decide():
            base = self.canonical_params()
            if mode == "gradient":
                newp = densify_by_gradient(base, state[0], state[1], grad_threshold if densify_ratio > 0.0 else math.inf,
                                           split_scale, max_gaussians, prune_opacity, self._dgen, keep=keep)
            elif mode == "error":
                op = torch.sigmoid(base["opacities_raw"].detach())
                kept = int(keep.sum()) if keep is not None else max(int((op > prune_opacity).sum()), min(64, n_now))
                newp = densify_by_error(base, err, error_threshold, split_scale, max_gaussians, prune_opacity,
                                        int(kept * densify_ratio) if densify_ratio > 0.0 else 0, self._dgen, keep=keep,
                                        report=self.error_report)
            elif on_device:
                newp = densify_and_prune_device(base, max_gaussians, densify_ratio, prune_opacity, self._dgen, keep=keep)
            else:
                newp = densify_and_prune(base, max_gaussians, densify_ratio, prune_opacity, keep=keep)
            perm = None
            if self.reorder and newp["means"].shape[0] >= 2:
                perm = morton_order(newp["means"])
                newp = {k: torch.nn.Parameter(v.detach()[perm].contiguous()) for k, v in newp.items()}
            return newp, perm

        if self.world > 1:
            # rank 0 decides, everyone receives the new tensors
            dev = self.params["means"].device
            if self.rank == 0:
                newp, perm = decide()
                n = torch.tensor([newp["means"].shape[0], int(perm is not None)], device=dev)
            else:
                n = torch.zeros(2, dtype=torch.int64, device=dev)
            dist.broadcast(n, 0, group=self.group)
            n_new, has_perm = int(n[0].item()), bool(n[1].item())
            if self.rank != 0:
                newp = {k: torch.nn.Parameter(torch.empty((n_new,) + tuple(v.shape[1:]), device=v.device))
                        for k, v in self.params.items()}
                perm = torch.empty(n_new, dtype=torch.int64, device=dev) if has_perm else None
            for k in sorted(newp):
                dist.broadcast(newp[k].data, 0, group=self.group)
            if has_perm:
                dist.broadcast(perm, 0, group=self.group)
            self.params, self.perm = newp, perm
        else:
            self.params, self.perm = decide()
        self.reset_optimizer()
        self._stats = []  # a new window of statistics, at the new size (made zeroed by the next step)


# ------------------------------------------------------------------------------------------------
# CLI: same flags as fit_multiview_stub.py:200-229.
# ------------------------------------------------------------------------------------------------
def _load_image(path: Path, width: int, height: int, gray: bool = False) -> np.ndarray:
    from PIL import Image

    img = Image.open(path).convert("L" if gray else "RGB").resize((width, height), Image.Resampling.BILINEAR)
    return np.asarray(img, dtype=np.float32) / 255.0


def _load_weights(wdir: Path, stem: str, width: int, height: int) -> torch.Tensor:
    """--weights_dir's map of one training view: <stem>.npy as it is (the fitter checks shape, dtype and values), else
    <stem>.png through _load_image (grey, 0..255 -> 0..1, resized like the targets)."""
    npy, png = wdir / f"{stem}.npy", wdir / f"{stem}.png"
    if npy.exists():
        return torch.from_numpy(np.load(npy))
    if png.exists():
        return torch.from_numpy(_load_image(png, width, height, gray=True))
    raise FileNotFoundError(f"--weights_dir: no weight map for training view '{stem}' ({npy.name} or {png.name}) in {wdir}")


def orbit_cameras(num_views: int, width: int, height: int, device) -> list:
    """fit_multiview_stub.py:70-90."""
    proj = tr.perspective(60.0, width / height, 0.01, 100.0, device=device)
    target = torch.tensor([0.0, 0.0, 0.0], dtype=torch.float32, device=device)
    up = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float32, device=device)
    cams = []
    for i in range(num_views):
        yaw = (2.0 * math.pi * i) / max(1, num_views)
        eye = torch.tensor([2.5 * math.cos(0.2) * math.sin(yaw), 2.5 * math.sin(0.2), 2.5 * math.cos(0.2) * math.cos(yaw)],
                           dtype=torch.float32, device=device)
        cams.append(tr.Camera(view=tr.look_at(eye, target, up), proj=proj))
    return cams


def main(argv=None) -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets_dir", required=True)
    ap.add_argument("--out_dir", default="outputs/fit_multiview_stub")
    ap.add_argument("--camera_npz", default="")
    ap.add_argument("--masks_dir", default="")
    ap.add_argument("--depth_dir", default="")
    ap.add_argument("--weights_dir", default="",
                    help="per-pixel loss weights of the training views: per target <stem>.npy (float32 (height, width), "
                         "any finite values >= 0), else <stem>.png (grey, 0..255 -> 0..1); every L1 term of a pixel counts "
                         "that many times (0: a pixel the fit does not see: a passer-by, sky, a lens flare); a training "
                         "view without a file is an error, held-out views need none; no D-SSIM term (--dssim_weight 0)")
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--lr", type=float, default=0.02)
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--height", type=int, default=128)
    ap.add_argument("--num_gaussians", type=int, default=800)
    ap.add_argument("--max_gaussians", type=int, default=3000)
    ap.add_argument("--use_sh", action="store_true")
    ap.add_argument("--sh_degree", type=int, default=1, choices=(1, 3), help="with --use_sh: 1 (reference) or 3 (extension)")
    ap.add_argument("--densify_interval", type=int, default=80)
    ap.add_argument("--prune_interval", type=int, default=80)
    ap.add_argument("--densify_ratio", type=float, default=0.15)
    ap.add_argument("--prune_opacity", type=float, default=0.05)
    ap.add_argument("--prune_mode", choices=("opacity", "contribution"), default="opacity",
                    help="opacity: the reference's rule (sigmoid(opacity) > --prune_opacity); contribution: keep a Gaussian "
                         "whose peak blend weight w / (1 + W) over the training views' pixels exceeds --prune_contribution "
                         "(what it owns of its best pixel under this renderer's weighted-average compositing)")
    ap.add_argument("--prune_contribution", type=float, default=1.0 / 510.0,
                    help="contribution mode: the peak blend weight t at or below which a Gaussian is pruned.  Removing one "
                         "such Gaussian moves no training pixel by more than t / (1 - t); the default 1/510 makes that "
                         "1/509, half an 8-bit level.  A bound per removed Gaussian, not a measured quality result")
    ap.add_argument("--densify_mode", choices=("opacity", "gradient", "error"), default="opacity",
                    help="opacity: the reference's rule (duplicate the most opaque Gaussians); gradient: adaptive density "
                         "control from each Gaussian's accumulated screen-space positional gradient (clone small, split "
                         "large, at most --max_gaussians); error: the same clone / split step on the Gaussians that own "
                         "the most L1 error, each pixel's error shared out by the blend weights w / (1 + W) and the "
                         "largest view taken, measured once per densify (nothing is collected during steps)")
    ap.add_argument("--densify_error_threshold", type=float, default=0.0,
                    help="error mode: only Gaussians whose blend-weighted error (pixels x colour error, largest view) "
                         "exceeds this are candidates.  The default 0 leaves the choice to the ranking and "
                         "--densify_ratio (the int(kept x ratio) largest); no default threshold has been measured")
    ap.add_argument("--densify_grad_threshold", type=float, default=0.0002,
                    help="gradient mode: densify where the mean NDC-position gradient norm per seeing view reaches this; "
                         "the default is the splatting trainers' convention, not measured for this renderer's "
                         "weighted-average compositing (DESIGN 8d records the distribution on the golden fit)")
    ap.add_argument("--densify_percent_dense", type=float, default=0.01,
                    help="gradient mode: split (not clone) above this fraction of the scene extent (1.1 x the largest "
                         "distance of a camera centre from their mean); the trainers' convention, not measured here")
    ap.add_argument("--silhouette_weight", type=float, default=0.2)
    ap.add_argument("--mask_thresh", type=float, default=0.06)
    ap.add_argument("--depth_weight", type=float, default=0.05)
    ap.add_argument("--dssim_weight", type=float, default=0.0,
                    help="l in (1 - l) L1 + l (1 - SSIM) for the photometric term (0: the reference's L1 fit)")
    ap.add_argument("--dssim_fused", action="store_true",
                    help="with --dssim_weight > 0 on the HIP device: the fused path's D-SSIM form (the D-SSIM backward "
                         "fused with the render backward's upstream pass) instead of the per-view autograd path")
    ap.add_argument("--reg_opacity", type=float, default=0.001)
    ap.add_argument("--reg_scale", type=float, default=0.001)
    ap.add_argument("--seed", type=int, default=None, help="torch.manual_seed before initialisation")
    ap.add_argument("--holdout_every", type=int, default=0,
                    help="K > 0: the views with index %% K == 0 (in the sorted target order) are kept out of the fit and "
                         "evaluated (PSNR / SSIM / L1 per view, eval.json); 0 (default): every view is fitted")
    ap.add_argument("--eval_interval", type=int, default=0,
                    help="M > 0: evaluate every M iterations and after the last (the held-out views, or without "
                         "--holdout_every the training views); 0 (default): once after the last iteration, and only "
                         "with --holdout_every")
    ap.add_argument("--eval_color_correct", action="store_true",
                    help="with an evaluation (--holdout_every / --eval_interval): also the colour-corrected metrics, "
                         "PSNR / SSIM / L1 of each view's render mapped onto its target by the view's best affine colour "
                         "transform (closed form; the cc_* keys of eval.json): a reading that per-view exposure and "
                         "white balance of the photos do not move")
    ap.add_argument("--eval_ridge", type=float, default=losses.CC_RIDGE,
                    help="with --eval_color_correct: the ridge that pulls the fitted transform towards the identity")
    ap.add_argument("--eval_masked", action="store_true",
                    help="with an evaluation (--holdout_every / --eval_interval): also the masked metrics, PSNR / SSIM / "
                         "L1 weighted by each evaluated view's mask (the object, not the background) and the silhouette's "
                         "L1 and IoU against it (the fg_* and sil_* keys of eval.json); needs masks: --masks_dir, or the "
                         "--mask_thresh rule with --silhouette_weight > 0")
    ap.add_argument("--refine_cameras", action="store_true",
                    help="fit the training views' poses with the Gaussians (a 6-vector per view, pose_view) and write "
                         "cameras_refined.npz (the --camera_npz schema)")
    ap.add_argument("--camera_lr", type=float, default=1e-3,
                    help="with --refine_cameras: Adam's learning rate of the pose deltas (chosen on the CPU dense renderer "
                         "at 64x48, not measured on the GPU or on real data)")
    ap.add_argument("--camera_fix", default="0",
                    help="with --refine_cameras: comma list of training-view indices whose poses stay as given (they pin "
                         "the scene's frame), or 'none'")
    ap.add_argument("--exposure", action="store_true",
                    help="fit a 3x4 exposure / white-balance transform per training view with the Gaussians (from "
                         "identity; the photometric term compares the transformed render with the target) and write "
                         "exposures.npz; host tensors (--device cpu), or the HIP device with --exposure_fused; held-out "
                         "metrics (--holdout_every) are taken without exposure: held-out views have none, and the metric is "
                         "of the image rendered from the saved Gaussians; --eval_color_correct is the way to judge "
                         "held-out views of such photo sets")
    ap.add_argument("--exposure_lr", type=float, default=1e-3,
                    help="with --exposure: Adam's learning rate of the exposure matrices")
    ap.add_argument("--exposure_fix", default="0",
                    help="with --exposure: comma list of training-view indices whose exposure stays at identity (they pin "
                         "the overall brightness), or 'none'")
    ap.add_argument("--exposure_fused", action="store_true",
                    help="with --exposure on the HIP device: the fused path's exposure form (the exposure matrices read "
                         "and their gradients written by the render backward's upstream pass; the Python schedule, no "
                         "D-SSIM term) instead of an error; changes nothing with --device cpu")
    ap.add_argument("--device", default="", help="cpu: host tensors (cpu_renderer, gloo); default: the HIP device")
    args = ap.parse_args(argv)
    if args.exposure_fused and not args.exposure:
        ap.error("--exposure_fused requires --exposure")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    on_host = args.device == "cpu" or not torch.cuda.is_available()
    if world > 1:
        if not on_host:
            torch.cuda.set_device(local_rank)
        dist.init_process_group("gloo" if on_host else "nccl")
    rank = dist.get_rank() if world > 1 else 0
    device = torch.device("cpu") if on_host else torch.device("cuda", local_rank)
    if args.seed is not None:
        torch.manual_seed(args.seed)
    if rank == 0:
        print(f"Using device: {device} (ranks: {world})")

    tdir = Path(args.targets_dir)
    paths = sorted([*tdir.glob("*.png"), *tdir.glob("*.jpg"), *tdir.glob("*.jpeg")])
    if not paths:
        raise FileNotFoundError(f"No target images found in {tdir} (supported: png/jpg/jpeg)")
    targets = [torch.from_numpy(_load_image(p, args.width, args.height)).to(device) for p in paths]
    masks = None
    if args.masks_dir:
        cand = [Path(args.masks_dir) / f"{p.stem}.png" for p in paths]
        if all(c.exists() for c in cand):
            masks = [torch.from_numpy(_load_image(c, args.width, args.height, gray=True)).to(device) for c in cand]
    if masks is None and args.silhouette_weight > 0.0:
        masks = [(t.mean(dim=2) > args.mask_thresh).to(torch.float32) for t in targets]
    if args.eval_masked and masks is None:
        raise ValueError("--eval_masked needs masks: --masks_dir with a mask per target, or --silhouette_weight > 0 (the "
                         "--mask_thresh rule)")
    depths = None
    if args.depth_dir:
        cand = [Path(args.depth_dir) / f"{p.stem}.png" for p in paths]
        if all(c.exists() for c in cand):
            depths = [torch.from_numpy(_load_image(c, args.width, args.height, gray=True)).to(device) for c in cand]
    if args.camera_npz:
        data = np.load(args.camera_npz)
        if "view" not in data or "proj" not in data:
            raise KeyError("camera npz must contain arrays: view (V,4,4), proj (V,4,4)")
        views, projs = np.asarray(data["view"], np.float32), np.asarray(data["proj"], np.float32)
        if views.shape[0] != len(targets) or projs.shape[0] != len(targets):
            raise ValueError("camera count mismatch with number of target images")
        cams = [tr.Camera(view=torch.from_numpy(views[i]).to(device), proj=torch.from_numpy(projs[i]).to(device))
                for i in range(len(targets))]
    else:
        cams = orbit_cameras(len(targets), args.width, args.height, device)

    all_cams = cams  # (the preview renders view 0 of all)
    hold = []
    train = list(range(len(targets)))
    if args.holdout_every < 0 or args.eval_interval < 0:
        raise ValueError("--holdout_every and --eval_interval must not be negative")
    if args.holdout_every > 0:
        # held-out views: out of the targets, cameras, masks, depths (and so of the densify extent below)
        hold = [i for i in range(len(targets)) if i % args.holdout_every == 0]
        train = [i for i in range(len(targets)) if i % args.holdout_every != 0]
        if not train:
            raise ValueError(f"--holdout_every {args.holdout_every} leaves no training view of {len(targets)}")
        eval_cams, eval_targets = [cams[i] for i in hold], [targets[i] for i in hold]
        eval_masks = [masks[i] for i in hold] if args.eval_masked else None
        pick = lambda xs: None if xs is None else [xs[i] for i in train]  # noqa: E731
        targets, masks, depths, cams = pick(targets), pick(masks), pick(depths), pick(cams)
    if args.weights_dir:  # the training views' loss weights (held-out views have none: evaluation is unweighted)
        refine_weights = [_load_weights(Path(args.weights_dir), paths[i].stem, args.width, args.height).to(device)
                          for i in train]
    do_eval = args.holdout_every > 0 or args.eval_interval > 0
    eval_log = [] if do_eval else None

    refine = {}
    if args.refine_cameras:
        fix = args.camera_fix.strip().lower()
        fixed = () if fix in ("none", "") else tuple(int(x) for x in fix.split(","))
        refine = dict(refine_cameras=True, camera_lr=args.camera_lr, camera_fixed=fixed)
        if rank == 0 and hold:
            print(f"refine_cameras: the {len(hold)} held-out views keep their input poses; the held-out metrics are "
                  "taken at those poses")
    if args.exposure:
        fix = args.exposure_fix.strip().lower()
        fixed = () if fix in ("none", "") else tuple(int(x) for x in fix.split(","))
        refine.update(exposure=True, exposure_lr=args.exposure_lr, exposure_fixed=fixed,
                      exposure_fused=args.exposure_fused)
    if args.weights_dir:
        refine.update(weights=refine_weights)
    params = build_params(args.num_gaussians, device, args.use_sh, args.sh_degree)
    fitter = ViewShardedFitter(params, cams, targets, args.width, args.height, lr=args.lr, masks=masks, depths=depths,
                               silhouette_weight=args.silhouette_weight, depth_weight=args.depth_weight,
                               reg_opacity=args.reg_opacity, reg_scale=args.reg_scale, dssim_weight=args.dssim_weight,
                               dssim_fused=args.dssim_fused, density_stats=args.densify_mode == "gradient",
                               **refine)
    centres = torch.stack([torch.linalg.inv(c.view.detach().float().cpu())[:3, 3] for c in cams])
    extent = 1.1 * float((centres - centres.mean(dim=0)).norm(dim=1).max())
    loss_log = []
    pending = []  # the step tensors not yet read: a replayed step found to have overflowed is redone and its loss
    #               rewritten in place one step later (graph_sync), so the host reads them after that
    for it in range(args.iters):
        pending.append(fitter.step())
        if rank == 0 and (it == 0 or (it + 1) % 25 == 0):
            fitter.graph_sync()
            print(f"iter {it+1:4d}  loss={float(pending[-1]):.6f}  N={fitter.params['means'].shape[0]}")
        if (it + 1) % args.prune_interval == 0 or (it + 1) % args.densify_interval == 0 or it + 1 == args.iters:
            fitter.graph_sync()
            loss_log.extend(float(t) for t in pending)
            pending = []
        if do_eval and ((args.eval_interval > 0 and (it + 1) % args.eval_interval == 0) or it + 1 == args.iters):
            # a collective (every rank); the held-out views if there are any, else the training views
            cc = dict(color_correct=True, ridge=args.eval_ridge) if args.eval_color_correct else {}
            if args.eval_masked:  # (the held-out views' own masks; the training views' are the fitter's)
                cc["masks"] = eval_masks if hold else True
            r = fitter.evaluate(eval_cams, eval_targets, **cc) if hold else fitter.evaluate(**cc)
            n_now = int(fitter.params["means"].shape[0])
            eval_log.append({"iter": it + 1, "n": n_now, "views": hold if hold else list(range(len(targets))),
                             "psnr": r["psnr"].tolist(), "ssim": r["ssim"].tolist(), "l1": r["l1"].tolist(),
                             "mean_psnr": r["mean_psnr"], "mean_ssim": r["mean_ssim"], "mean_l1": r["mean_l1"]})
            if args.eval_color_correct:
                for k in ("psnr", "ssim", "l1"):
                    eval_log[-1].update({"cc_" + k: r["cc_" + k].tolist(), "mean_cc_" + k: r["mean_cc_" + k]})
                eval_log[-1]["cc_transform"] = r["cc_transform"].tolist()
            if args.eval_masked:
                for k in ("fg_fraction", "fg_psnr", "fg_ssim", "fg_l1", "sil_l1", "sil_iou"):
                    eval_log[-1].update({k: r[k].tolist(), "mean_" + k: r["mean_" + k]})
            if rank == 0:
                print(f"eval iter {it+1:4d}  N={n_now}  PSNR={r['mean_psnr']:.3f} dB  SSIM={r['mean_ssim']:.5f}  "
                      f"L1={r['mean_l1']:.6f}  ({'held-out' if hold else 'training'} views: {len(r['psnr'])})")
                if args.eval_color_correct:
                    print(f"eval iter {it+1:4d}  colour-corrected: PSNR={r['mean_cc_psnr']:.3f} dB  "
                          f"SSIM={r['mean_cc_ssim']:.5f}  L1={r['mean_cc_l1']:.6f}")
                if args.eval_masked:
                    print(f"eval iter {it+1:4d}  masked: PSNR={r['mean_fg_psnr']:.3f} dB  SSIM={r['mean_fg_ssim']:.5f}  "
                          f"L1={r['mean_fg_l1']:.6f}  silhouette L1={r['mean_sil_l1']:.6f}  IoU={r['mean_sil_iou']:.5f}")
        if (it + 1) % args.prune_interval == 0 or (it + 1) % args.densify_interval == 0:
            fitter.densify_and_prune(args.max_gaussians,
                                     args.densify_ratio if (it + 1) % args.densify_interval == 0 else 0.0,
                                     args.prune_opacity, mode=args.densify_mode,
                                     grad_threshold=args.densify_grad_threshold,
                                     split_scale=args.densify_percent_dense * extent, prune_mode=args.prune_mode,
                                     prune_contribution=args.prune_contribution,
                                     error_threshold=args.densify_error_threshold)
            if rank == 0 and args.prune_mode == "contribution":
                r = fitter.contribution_report
                print(f"prune at iter {it + 1}: peak blend weight of {r['n']} Gaussians: p1={r['p1']:.3e} p10={r['p10']:.3e} "
                      f"p50={r['p50']:.3e}, {r['at_or_below']} at or below {r['threshold']:.3e} ({r['pruned']} pruned); the "
                      f"opacity rule ({args.prune_opacity:g}) would have pruned {r['opacity_would_prune']} ({r['both']} in "
                      f"common); N -> {fitter.params['means'].shape[0]}")
            if rank == 0 and args.densify_mode == "gradient":
                r = fitter.density_report
                print(f"densify at iter {it + 1}: avg gradient over {r['seen']} of {r['n']} Gaussians seen: p50={r['p50']:.3e} "
                      f"p90={r['p90']:.3e} p99={r['p99']:.3e} max={r['max']:.3e}, {r['over']} at or over "
                      f"{args.densify_grad_threshold:g}; N -> {fitter.params['means'].shape[0]}")
            if rank == 0 and args.densify_mode == "error":
                r = fitter.error_report
                print(f"densify at iter {it + 1}: blend-weighted error of {r['n']} Gaussians: p50={r['p50']:.3e} "
                      f"p90={r['p90']:.3e} p99={r['p99']:.3e} max={r['max']:.3e}, {r['over']} over {r['threshold']:g}; "
                      f"{r['clones']} cloned, {r['splits']} split; N -> {fitter.params['means'].shape[0]}")
    if args.refine_cameras:  # all input views in input order: the training views refined, the held-out ones as given
        all_cams = list(all_cams)
        for i, cam in zip(train, fitter.refined_cameras()):
            all_cams[i] = cam
    if rank == 0:
        save_outputs(fitter, all_cams, args, Path(args.out_dir), loss_log, eval_log)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def save_outputs(fitter: ViewShardedFitter, cams, args, out_dir: Path, loss_log, eval_log=None) -> None:
    """gaussians_fitted.npz / loss.txt / preview_view0.png exactly as fit_multiview_stub.py:327-380; with ``eval_log``
    (--holdout_every / --eval_interval: one dict per evaluation) also eval.json."""
    from PIL import Image

    out_dir.mkdir(parents=True, exist_ok=True)
    p = fitter.canonical_params()
    means = p["means"]
    scales = torch.nn.functional.softplus(p["scales_raw"]) + 1e-3
    opacities = torch.sigmoid(p["opacities_raw"])
    sh = p.get("sh_raw")
    colors = sh[:, 0, :].clamp(0.0, 1.0) if sh is not None else torch.sigmoid(p["colors_raw"])
    arrays = dict(means=means, scales=scales, colors=colors, opacities=opacities)
    if sh is not None:
        arrays["sh_coeffs"] = sh
    if getattr(args, "dssim_weight", 0.0) > 0.0:
        # the loss the Gaussians were fitted with (absent: the reference's L1 fit, whose file is unchanged)
        arrays["dssim_weight"] = torch.tensor(float(args.dssim_weight))
    np.savez(out_dir / "gaussians_fitted.npz", **{k: v.detach().cpu().numpy().astype(np.float32) for k, v in arrays.items()})
    (out_dir / "loss.txt").write_text("\n".join(f"{v:.8f}" for v in loss_log), encoding="utf-8")
    if eval_log is not None:
        (out_dir / "eval.json").write_text(json.dumps(eval_log, indent=1), encoding="utf-8")
    if getattr(args, "refine_cameras", False):  # the --camera_npz schema: feed it back with --camera_npz
        np.savez(out_dir / "cameras_refined.npz",
                 view=np.stack([c.view.detach().cpu().numpy().astype(np.float32) for c in cams]),
                 proj=np.stack([c.proj.detach().cpu().numpy().astype(np.float32) for c in cams]))
    if getattr(args, "exposure", False):  # the training views' exposure matrices, in their order
        np.savez(out_dir / "exposures.npz", exposure=fitter.exposure_state()[0].numpy().astype(np.float32))
    with torch.no_grad():
        pred0 = tr.render_gaussians_torch(means, scales, sh if sh is not None else colors, opacities, cams[0],
                                          width=args.width, height=args.height,
                                          background=torch.tensor([0.0, 0.0, 0.0], device=means.device),
                                          max_gaussians=max(args.max_gaussians, means.shape[0]), return_aux=False)
        Image.fromarray((pred0.clamp(0, 1).cpu().numpy() * 255.0).astype(np.uint8), mode="RGB").save(out_dir / "preview_view0.png")
    print(f"Done. Outputs written to: {out_dir}")


if __name__ == "__main__":
    main()
