"""GPU: the view backward's entries agree with each other bit for bit where they run the same launches (bwd_impl serves
all of them from one request): a full entry equals its gather entry followed by a one-view gr_reduce_sums, written and
added; gr_bwd_fit_ssim at w_dssim = 0 equals gr_bwd_fit; gr_bwd_indexed with the identity index equals gr_bwd.

One view at 40 x 24 (3 x 2 tiles, both edges partial), n = 257 (one past a 256-thread block and past four 64-row gather
blocks), colour dims 3 and 12, masks on."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

W, H, N = 40, 24, 257
W_SIL, W_DEPTH, G_SCALE, W_DSSIM = 0.2, 0.05, 0.25, 0.2

_STATES: dict = {}


def _state(pkg, cuda, cd, depth):
    """The view rendered once per colour dim and depth mode (shared by the tests, left unchanged)."""
    key = (cd, depth)
    if key not in _STATES:
        tr = pkg.torch_renderer
        sc = orc.synthetic_scene(N, seed=1)
        colors = sc.colors
        if cd != 3:
            rng = np.random.default_rng(N + cd)
            colors = (rng.standard_normal((N, cd // 3, 3)) * 0.3).astype(np.float32)
            colors[:, 0, :] += 0.5
        p = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in (sc.means, sc.scales, colors, sc.opacities))
        view, proj = orc.orbit_cameras(8, W, H)[1]
        g = torch.Generator(device=cuda).manual_seed(12)
        target = torch.rand((H, W, 3), generator=g, device=cuda)
        mask = (target.mean(dim=2) > 0.5).float().contiguous()
        tdepth = torch.rand((H, W), generator=g, device=cuda)
        ups = (torch.randn((H, W, 3), generator=g, device=cuda), torch.randn((H, W), generator=g, device=cuda),
               torch.randn((H, W), generator=g, device=cuda))
        gv = tr.make_view(view, proj, W, H, None, depth_grad=depth)
        _, _, _, st = tr.forward_native(*p, gv, tr.prepare_native(*p, gv))
        torch.cuda.synchronize()
        assert st.plan.num_pairs > 0
        _STATES[key] = dict(p=p, st=st, target=target, mask=mask, tdepth=tdepth, ups=ups)
    return _STATES[key]


def _buffers(S, accumulate):
    return tuple(torch.full_like(t, 0.5) if accumulate else torch.full_like(t, float("nan")) for t in S["p"])


def _full(tr, S, entry, depth, grads, accumulate):
    """The full entry into grads; returns its loss."""
    loss = torch.zeros(1, device=grads[0].device)
    td, wd = (S["tdepth"], W_DEPTH) if depth else (None, 0.0)
    if entry == "l1":
        tr.backward_l1_native(*S["p"], S["st"], S["target"], S["mask"], W_SIL, G_SCALE, loss, grads, accumulate)
    elif entry == "fit":
        tr.backward_fit_native(*S["p"], S["st"], S["target"], S["mask"], W_SIL, td, wd, G_SCALE, loss, grads, accumulate)
    else:
        lam = W_DSSIM if entry == "ssim" else 0.0
        tr.backward_fit_ssim_native(*S["p"], S["st"], S["target"], S["mask"], W_SIL, td, wd, G_SCALE, lam, loss, grads, accumulate)
    return loss


def _gathered(tr, S, entry, depth, grads, accumulate):
    """The entry's gather entry, then gr_reduce_sums of that one view into grads; returns the loss.  gr_bwd_l1 has no
    gather entry of its own: its sums are gr_bwd_fit_ssim_gather's at w_dssim = 0 without a depth target."""
    loss = torch.zeros(1, device=grads[0].device)
    td, wd = (S["tdepth"], W_DEPTH) if depth else (None, 0.0)
    if entry == "fit":
        sums, sums3 = tr.backward_fit_gather_native(S["st"], S["target"], S["mask"], W_SIL, td, wd, G_SCALE, loss)
    else:
        lam = W_DSSIM if entry == "ssim" else 0.0
        sums, sums3 = tr.backward_fit_ssim_gather_native(S["st"], S["target"], S["mask"], W_SIL, td, wd, G_SCALE, lam, loss)
    view = (S["st"].gv, sums, sums3) if depth else (S["st"].gv, sums)
    tr.reduce_sums_native(*S["p"], [view], grads, accumulate)
    return loss


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b)) and all(bool(torch.isfinite(x).all()) for x in a)


@pytest.mark.parametrize("entry,depth", [("l1", False), ("fit", False), ("fit", True), ("ssim", False), ("ssim", True)],
                         ids=["gr_bwd_l1", "gr_bwd_fit", "gr_bwd_fit-depth", "gr_bwd_fit_ssim", "gr_bwd_fit_ssim-depth"])
@pytest.mark.parametrize("cd", [3, 12])
def test_full_entry_equals_gather_then_one_view_reduce(pkg, cuda, cd, entry, depth):
    tr = pkg.torch_renderer
    S = _state(pkg, cuda, cd, depth)
    for accumulate in (False, True):
        ga, gb = _buffers(S, accumulate), _buffers(S, accumulate)
        la = _full(tr, S, entry, depth, ga, accumulate)
        lb = _gathered(tr, S, entry, depth, gb, accumulate)
        torch.cuda.synchronize()
        assert torch.equal(la, lb) and float(la) > 0.0, accumulate
        assert _same(ga, gb), accumulate
        assert float((ga[0] - (0.5 if accumulate else 0.0)).abs().max()) > 0.0


@pytest.mark.parametrize("depth", [False, True], ids=["rgb-only", "depth"])
@pytest.mark.parametrize("cd", [3, 12])
def test_ssim_entry_at_zero_weight_equals_gr_bwd_fit(pkg, cuda, cd, depth):
    tr = pkg.torch_renderer
    S = _state(pkg, cuda, cd, depth)
    for accumulate in (False, True):
        ga, gb = _buffers(S, accumulate), _buffers(S, accumulate)
        la = _full(tr, S, "fit", depth, ga, accumulate)
        lb = _full(tr, S, "ssim0", depth, gb, accumulate)
        torch.cuda.synchronize()
        assert torch.equal(la, lb) and _same(ga, gb), accumulate


@pytest.mark.parametrize("depth", [False, True], ids=["rgb-only", "depth"])
@pytest.mark.parametrize("cd", [3, 12])
def test_identity_index_equals_gr_bwd(pkg, cuda, cd, depth):
    tr = pkg.torch_renderer
    S = _state(pkg, cuda, cd, depth)
    g_rgb, g_alpha, g_depth = S["ups"]
    ups = (g_rgb, g_alpha, g_depth if depth else None)
    index = torch.arange(N, dtype=torch.int32, device=cuda)
    ga = tr.backward_native(*S["p"], S["st"], *ups)
    gb = tr.backward_native(*S["p"], S["st"], *ups, index=index)
    torch.cuda.synchronize()
    assert _same(ga, gb) and float(ga[0].abs().max()) > 0.0
