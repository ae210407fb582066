"""GPU, kernel level: the fused D-SSIM fit backward (gr_bwd_fit_ssim / gr_bwd_fit_ssim_gather: k_ssim_fwd_saved +
k_ssim_pixel_grads in libgr_hip.so) against the chain composed from the entries that existed before it:
forward_native(images=True), the loss in torch through losses.l1_loss / losses.dssim_loss, autograd.grad for the
upstream images, then gr_bwd on the same forward state.

Margin per parameter tensor: max|g_fused - g_composed| <= max(4 b, 1e-6 max|g_composed|), b the same difference at
l = 0 between gr_bwd_fit and the composed chain (both older code), measured in the same test; the loss within
1e-6 max(1, |loss|).
"""
from __future__ import annotations

import ctypes
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

W_SIL, W_DEPTH, G_SCALE = 0.2, 0.05, 0.25
NAMES = ("d_means", "d_scales", "d_colors", "d_opacities")


@pytest.fixture(scope="module")
def mods(pkg, cuda):
    return (importlib.import_module("3dgaussian_amd.torch_renderer"), importlib.import_module("3dgaussian_amd.fit_multiview"),
            importlib.import_module("3dgaussian_amd.losses"), importlib.import_module("bench"))


_STATES: dict = {}


def _state(mods, cuda, W, H, n, depth=False, bg=None, shift=0.0):
    """One view of n Gaussians rendered once (shared by the tests, left unchanged): parameters, targets, forward."""
    key = (W, H, n, depth, bg, shift)
    if key not in _STATES:
        tr, fm, _, bench = mods
        p = bench.synthetic_params(n, cuda)
        with torch.no_grad():
            p["colors_raw"].add_(1.5)  # visible colours (the synthetic ones are near black)
            p["means"].add_(torch.tensor([0.0, shift, 0.0], device=cuda))  # (far above every orbit camera's view)
        m, s, c, o = (t.detach().contiguous() for t in fm.activations(p))
        cam = fm.orbit_cameras(3, W, H, cuda)[1]
        g = torch.Generator().manual_seed(11)
        target = torch.rand((H, W, 3), generator=g).to(cuda)
        mask = (torch.rand((H, W), generator=g) > 0.5).float().to(cuda)
        tdepth = torch.rand((H, W), generator=g).to(cuda)
        gv = tr.make_view(cam.view, cam.proj, W, H, list(bg) if bg else None, depth_grad=depth)
        out, alpha, dimg, st = tr.forward_native(m, s, c, o, gv)
        torch.cuda.synchronize()
        _STATES[key] = dict(p=(m, s, c, o), target=target, mask=mask, tdepth=tdepth, out=out, alpha=alpha, depth=dimg, st=st)
    return _STATES[key]


def _composed(mods, S, lam, use_mask, use_depth):
    """(unscaled loss, gradients) of the composed chain."""
    tr, _, losses, _ = mods
    pred = S["out"].clone().requires_grad_(True)
    a = S["alpha"].clone().requires_grad_(True)
    d = S["depth"].clone().requires_grad_(True) if use_depth else None
    val = (1.0 - lam) * losses.l1_loss(pred, S["target"])
    if lam > 0.0:
        val = val + lam * losses.dssim_loss(pred, S["target"])
    if use_mask:
        val = val + W_SIL * losses.l1_loss(a, S["mask"])
    if use_depth:
        val = val + W_DEPTH * torch.mean(torch.abs(d / (d.max() + 1e-6) - S["tdepth"]))
    ins = [pred] + ([a] if use_mask else []) + ([d] if use_depth else [])
    gs = list(torch.autograd.grad(G_SCALE * val, ins))
    g_rgb = gs.pop(0).contiguous()
    g_alpha = gs.pop(0).contiguous() if use_mask else None
    g_depth = gs.pop(0).contiguous() if use_depth else None
    return float(val.detach()), tr.backward_native(*S["p"], S["st"], g_rgb, g_alpha, g_depth)


def _fused(mods, S, lam, use_mask, use_depth, grads=None, accumulate=False, ssim_entry=True):
    tr = mods[0]
    loss = torch.zeros(1, device=S["out"].device)
    if grads is None:
        grads = tuple(torch.empty_like(t) for t in S["p"])
    mask = S["mask"] if use_mask else None
    td = S["tdepth"] if use_depth else None
    wd = W_DEPTH if use_depth else 0.0
    if ssim_entry:
        tr.backward_fit_ssim_native(*S["p"], S["st"], S["target"], mask, W_SIL, td, wd, G_SCALE, lam, loss, grads, accumulate)
    else:
        tr.backward_fit_native(*S["p"], S["st"], S["target"], mask, W_SIL, td, wd, G_SCALE, loss, grads, accumulate)
    return loss, grads


CASES = [
    # W, H, n, mask, depth, background
    (50, 37, 1500, True, False, None),   # partial tiles on both edges, an interior tile with all eight neighbours
    (50, 37, 1500, False, False, None),
    (50, 37, 1500, True, True, None),    # a depth target (no_depth_grad = 0)
    (50, 37, 1500, False, False, (0.2, 0.5, 0.7)),
    (16, 16, 400, True, False, None),    # exactly one tile
    (16, 16, 400, False, False, None),
    (7, 5, 200, True, False, None),      # smaller than the tile and the window
    (7, 5, 200, False, False, None),
]


@pytest.mark.parametrize("W,H,n,use_mask,use_depth,bg", CASES,
                         ids=[f"{c[0]}x{c[1]}{'-mask' if c[3] else ''}{'-depth' if c[4] else ''}{'-bg' if c[5] else ''}" for c in CASES])
def test_matches_composed_chain(mods, cuda, W, H, n, use_mask, use_depth, bg):
    S = _state(mods, cuda, W, H, n, use_depth, bg)
    assert S["st"].num_pairs > 0
    _, g0 = _composed(mods, S, 0.0, use_mask, use_depth)
    _, f0 = _fused(mods, S, 0.0, use_mask, use_depth, ssim_entry=False)  # gr_bwd_fit
    base = [float((a - b).abs().max()) for a, b in zip(f0, g0)]
    for lam in (0.2, 1.0):
        val, gc = _composed(mods, S, lam, use_mask, use_depth)
        loss, gf = _fused(mods, S, lam, use_mask, use_depth)
        torch.cuda.synchronize()
        dl = abs(float(loss) - val)
        print(f"dssim fused {W}x{H} l={lam}: loss {float(loss):.7f} composed {val:.7f} diff {dl:.2e}")
        ok = dl <= 1e-6 * max(1.0, abs(val))
        for name, a, b, b0 in zip(NAMES, gf, gc, base):
            d, gmax = float((a - b).abs().max()), float(b.abs().max())
            bound = max(4.0 * b0, 1e-6 * gmax)
            print(f"  {name}: diff {d:.3e} (l = 0: {b0:.3e}) max|g| {gmax:.3e} bound {bound:.3e}")
            assert torch.isfinite(a).all()
            ok = ok and d <= bound
        assert ok and float(gc[0].abs().max()) > 0.0  # (a 7 x 5 view clamps every sigma: its scale gradients are zero)


@pytest.mark.parametrize("use_depth", [False, True])
def test_zero_weight_is_gr_bwd_fit(mods, cuda, use_depth):
    tr = mods[0]
    S = _state(mods, cuda, 50, 37, 1500, use_depth)
    l0, g0 = _fused(mods, S, 0.0, True, use_depth, ssim_entry=False)
    l1, g1 = _fused(mods, S, 0.0, True, use_depth)
    assert torch.equal(l0, l1)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
    td, wd = (S["tdepth"], W_DEPTH) if use_depth else (None, 0.0)
    la, lb = torch.zeros(1, device=cuda), torch.zeros(1, device=cuda)
    sa, sa3 = tr.backward_fit_gather_native(S["st"], S["target"], S["mask"], W_SIL, td, wd, G_SCALE, la)
    sb, sb3 = tr.backward_fit_ssim_gather_native(S["st"], S["target"], S["mask"], W_SIL, td, wd, G_SCALE, 0.0, lb)
    assert torch.equal(la, lb) and torch.equal(sa, sb)
    if use_depth:
        assert torch.equal(sa3, sb3)


@pytest.mark.parametrize("use_depth", [False, True])
def test_gather_and_reduce_is_the_full_backward(mods, cuda, use_depth):
    """gr_bwd_fit_ssim_gather + gr_reduce_sums of one view are gr_bwd_fit_ssim's two stages; accumulate adds; two runs
    are equal."""
    tr = mods[0]
    S = _state(mods, cuda, 50, 37, 1500, use_depth)
    lam = 0.2
    loss, full = _fused(mods, S, lam, True, use_depth)
    loss2, full2 = _fused(mods, S, lam, True, use_depth)
    assert torch.equal(loss, loss2)
    for a, b in zip(full, full2):
        assert torch.equal(a, b)
    td, wd = (S["tdepth"], W_DEPTH) if use_depth else (None, 0.0)
    lg = torch.zeros(1, device=cuda)
    sums, sums3 = tr.backward_fit_ssim_gather_native(S["st"], S["target"], S["mask"], W_SIL, td, wd, G_SCALE, lam, lg)
    assert (sums3 is not None) == use_depth
    got = tuple(torch.empty_like(t) for t in S["p"])
    item = (S["st"].gv, sums, sums3) if use_depth else (S["st"].gv, sums)
    tr.reduce_sums_native(*S["p"], [item], got, accumulate=False)
    assert torch.equal(lg, loss)
    for a, b in zip(got, full):
        assert torch.equal(a, b)
    acc = tuple(torch.full_like(t, 0.5) for t in S["p"])
    _fused(mods, S, lam, True, use_depth, grads=acc, accumulate=True)
    for a, b in zip(acc, full):
        torch.testing.assert_close(a, b + 0.5, rtol=1e-6, atol=1e-7)


def test_view_without_pairs(mods, cuda):
    """A camera that sees no Gaussian: the loss of the background image, zero sums."""
    tr, _, losses, _ = mods
    bg = (0.2, 0.5, 0.7)
    S = _state(mods, cuda, 50, 37, 300, False, bg, shift=1000.0)
    assert S["st"].num_pairs == 0
    lam = 0.2
    image = torch.tensor(bg, device=cuda).expand(37, 50, 3).contiguous()
    assert torch.equal(S["out"], image)
    val = float((1.0 - lam) * losses.l1_loss(image, S["target"]) + lam * losses.dssim_loss(image, S["target"])
                + W_SIL * losses.l1_loss(torch.zeros((37, 50), device=cuda), S["mask"]))
    loss = torch.zeros(1, device=cuda)
    sums, _ = tr.backward_fit_ssim_gather_native(S["st"], S["target"], S["mask"], W_SIL, None, 0.0, G_SCALE, lam, loss)
    torch.cuda.synchronize()
    assert abs(float(loss) - val) <= 1e-6 * max(1.0, abs(val))
    assert not sums.any()


def test_errors(mods, cuda):
    tr = mods[0]
    nat = tr._native
    L = nat.lib()
    S = _state(mods, cuda, 50, 37, 1500)
    st = S["st"]
    need = int(L.gr_bwd_ssim_bytes(ctypes.byref(st.gv), st.n, ctypes.byref(st.plan)))
    assert need >= int(L.gr_bwd_bytes(ctypes.byref(st.gv), st.n, ctypes.byref(st.plan))) + int(L.gr_ssim_ws_bytes(37, 50, 3, 1))
    ws = torch.zeros((need,), dtype=torch.uint8, device=cuda)
    loss = torch.zeros(1, device=cuda)
    sums = torch.zeros((st.n, 8), device=cuda)
    stream = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)

    def call(gv, lam, ws_bytes):
        return L.gr_bwd_fit_ssim_gather(ctypes.byref(gv), st.n, ctypes.byref(st.plan), nat.ptr(st.geom), nat.ptr(st.bins),
                                        nat.ptr(st.saved), nat.ptr(S["target"]), nat.ptr(S["mask"]), ctypes.c_float(W_SIL),
                                        None, ctypes.c_float(0.0), ctypes.c_float(G_SCALE), ctypes.c_float(lam),
                                        nat.ptr(loss), nat.ptr(ws), ws_bytes, nat.ptr(sums), None, stream)

    assert call(st.gv, 0.2, need - 1) == nat.GR_ERR_WORKSPACE and b"workspace" in L.gr_last_error()
    assert call(st.gv, 1.5, need) == nat.GR_ERR_INVALID_ARGUMENT and b"w_dssim" in L.gr_last_error()
    assert call(st.gv, -0.1, need) == nat.GR_ERR_INVALID_ARGUMENT
    t32 = nat.GrView.from_buffer_copy(st.gv)
    t32.tile = 32
    assert call(t32, 0.2, need) == nat.GR_ERR_INVALID_ARGUMENT
    band = nat.GrView.from_buffer_copy(st.gv)
    band.row0, band.rows = 0, 1
    assert call(band, 0.2, need) == nat.GR_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        tr.backward_fit_ssim_gather_native(st, S["target"], S["mask"], W_SIL, None, 0.0, G_SCALE, 1.5, loss)
    torch.cuda.synchronize()
    assert not sums.any() and float(loss) == 0.0  # a rejected call launches nothing
