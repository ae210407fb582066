"""GPU: the HIP device's exposure form.  Kernel level: gr_bwd_fit_exposure_gather (k_pixel_grads_expo in libgr_hip.so)
against gr_bwd_fit_gather at identity exposure (bit for bit), against the float64 restatement
tests/exposure_reference.py on the kernel's own saved sums (d loss / d E and the loss), against the chain composed
from the older entries (forward image -> exposed colour and loss in torch -> autograd -> gr_bwd) for the Gaussians'
gradients; determinism; refusals.  Fitter level: ViewShardedFitter(exposure=True, exposure_fused=True) on the Python
schedule against a fitter without exposure (identity on fixed views), against the dense float64 reference, recovery
of known exposures, fixed rows, and beside refine_cameras / density_stats.

Measured on an MI355X (printed by the tests; bars in brackets):
  d loss / d E against float64 on the kernel's sums: relL2 1.8e-8 .. 5.1e-8 [1e-4]; the loss within 3.4e-8 [1e-6]
  Gaussian gradients against the composed chain: equal bit for bit without a depth term (b0, identity E through
    gr_bwd_fit, is 0 there too); with one, max diff 2.4e-9 / 6.3e-9 / 0 / 3.7e-10 (means / scales / colours /
    opacities) beside b0 2.6e-9 / 6.1e-9 / 0 / 3.6e-10 [4 b0]
  fitter d loss / d E against the dense float64 reference: relL2 3.0e-8, the render's own d0 1.7e-6 [4 d0]
  recovery: mean |E - E_true| ratio 0.387 after 80 steps [0.5; host tensors: 0.387]
"""
from __future__ import annotations

import ctypes
import importlib
import os
import sys

import pytest
import torch

from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import exposure_reference as eref  # noqa: E402

pytestmark = pytest.mark.gpu

W_SIL, W_DEPTH, G_SCALE = 0.2, 0.05, 0.25
NAMES = ("d_means", "d_scales", "d_colors", "d_opacities")
GRAD_TOL = 1e-4  # tests/test_exposure_cpu.py's bar for d loss / d E: relative L2
EYE = torch.cat([torch.eye(3), torch.zeros(3, 1)], dim=1)


@pytest.fixture(scope="module")
def mods(pkg, cuda):
    return (importlib.import_module("3dgaussian_amd.torch_renderer"), importlib.import_module("3dgaussian_amd.fit_multiview"),
            importlib.import_module("3dgaussian_amd.losses"), importlib.import_module("bench"))


def _host_sums(st, W, H):
    """The view's saved sums on the host: (W, C_r, C_g, C_b) per pixel, then D -> (Wt (H, W), C (H, W, 3), D (H, W))."""
    sv = st.saved.detach().cpu()
    s4 = sv[:4 * W * H].view(H, W, 4)
    return s4[..., 0].clone(), s4[..., 1:4].clone(), sv[4 * W * H:5 * W * H].view(H, W).clone()


_STATES: dict = {}


def _state(mods, cuda, W, H, n, depth=False, bg=None, shift=0.0, e=1):
    """One view of n Gaussians rendered once (shared by the tests, left unchanged): parameters, forward, a non-trivial
    exposure E and targets kept 1e-3 from the kinks of |y - t| at that E and at identity."""
    key = (W, H, n, depth, bg, shift, e)
    if key not in _STATES:
        tr, fm, _, bench = mods
        p = bench.synthetic_params(n, cuda)
        with torch.no_grad():
            p["colors_raw"].add_(1.5)  # visible colours (the synthetic ones are near black)
            p["means"].add_(torch.tensor([0.0, shift, 0.0], device=cuda))  # (far above every orbit camera's view)
        m, s, c, o = (t.detach().contiguous() for t in fm.activations(p))
        cam = fm.orbit_cameras(3, W, H, cuda)[1]
        g = torch.Generator().manual_seed(11)
        target = torch.rand((H, W, 3), generator=g)
        mask = (torch.rand((H, W), generator=g) > 0.5).float().to(cuda)
        tdepth = torch.rand((H, W), generator=g).to(cuda)
        gv = tr.make_view(cam.view, cam.proj, W, H, list(bg) if bg else None, depth_grad=depth)
        out, alpha, dimg, st = tr.forward_native(m, s, c, o, gv)
        torch.cuda.synchronize()
        E = eref.true_exposures(20 + e)[e].contiguous()
        sums = _host_sums(st, W, H)
        bgt = None if bg is None else torch.tensor(bg)
        for _ in range(3):  # (a value pushed off one kink may land by another: a second and third pass)
            for Ek in (E, EYE):  # (identity: the composed chain's base b0 takes the plain loss's signs on the same target)
                target = eref.clear_targets(eref.exposed(sums, bgt, Ek)[0], target)
        for Ek in (E, EYE):
            assert float((eref.exposed(sums, bgt, Ek)[0] - target.double()).abs().min()) >= 0.9e-3
        _STATES[key] = dict(p=(m, s, c, o), target=target.to(cuda), mask=mask, tdepth=tdepth, out=out, alpha=alpha, depth=dimg,
                            st=st, E=E.to(cuda), sums=sums, bg=bgt, W=W, H=H)
    return _STATES[key]


def _expo(mods, S, E, use_mask, use_depth):
    """gr_bwd_fit_exposure_gather on the state: (loss, d_exposure, sums, sums3)."""
    tr = mods[0]
    dev = S["out"].device
    loss, dE = torch.zeros(1, device=dev), torch.full((12,), 7.0, device=dev)
    sums, sums3 = tr.backward_fit_exposure_gather_native(
        S["st"], S["target"], S["mask"] if use_mask else None, W_SIL, S["tdepth"] if use_depth else None,
        W_DEPTH if use_depth else 0.0, G_SCALE, E, dE, loss)
    return loss, dE, sums, sums3


def _reference(S, E, use_mask, use_depth):
    return eref.view_loss(S["sums"], S["bg"], E, S["target"], S["mask"] if use_mask else None, W_SIL,
                          S["tdepth"] if use_depth else None, W_DEPTH, G_SCALE)


CASES = [
    # W, H, n, mask, depth, background, shift
    (50, 37, 1500, True, False, None, 0.0),   # partial tiles on both edges, 12 tiles: the fan-in crosses blocks
    (50, 37, 1500, False, False, None, 0.0),
    (50, 37, 1500, True, True, None, 0.0),    # a depth target (no_depth_grad = 0)
    (50, 37, 1500, True, False, (0.2, 0.5, 0.7), 0.0),
    (16, 16, 400, True, False, None, 0.0),    # exactly one tile: the elected block is the only one
    (7, 5, 200, True, False, None, 0.0),      # smaller than a tile
    (50, 37, 300, True, False, (0.2, 0.5, 0.7), 1000.0),  # out of sight: num_pairs == 0
]
IDS = [f"{c[0]}x{c[1]}{'-mask' if c[3] else ''}{'-depth' if c[4] else ''}{'-bg' if c[5] else ''}{'-nopairs' if c[6] else ''}"
       for c in CASES]


# ---- 1. identity is today's entry, bit for bit --------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,n,use_mask,use_depth,bg,shift", CASES, ids=IDS)
def test_identity_is_gr_bwd_fit_gather(mods, cuda, W, H, n, use_mask, use_depth, bg, shift):
    tr = mods[0]
    S = _state(mods, cuda, W, H, n, use_depth, bg, shift)
    assert (S["st"].num_pairs == 0) == (shift != 0.0)
    td, wd = (S["tdepth"], W_DEPTH) if use_depth else (None, 0.0)
    la = torch.zeros(1, device=cuda)
    sa, sa3 = tr.backward_fit_gather_native(S["st"], S["target"], S["mask"] if use_mask else None, W_SIL, td, wd, G_SCALE, la)
    lb, dE, sb, sb3 = _expo(mods, S, EYE.to(cuda), use_mask, use_depth)
    torch.cuda.synchronize()
    assert float(la) > 0.0 and torch.equal(la, lb) and torch.equal(sa, sb)
    assert (sb3 is not None) == use_depth
    if use_depth:
        assert torch.equal(sa3, sb3)
    else:
        assert not sa3.any()
    assert torch.isfinite(dE).all() and float(dE.abs().max()) > 0.0 and not (dE == 7.0).any()


# ---- 2. d loss / d E against float64 on the kernel's own sums ------------------------------------------------------------
@pytest.mark.parametrize("W,H,n,use_mask,use_depth,bg,shift", CASES, ids=IDS)
def test_d_exposure_matches_float64(mods, cuda, W, H, n, use_mask, use_depth, bg, shift):
    S = _state(mods, cuda, W, H, n, use_depth, bg, shift)
    loss, dE, sums, _ = _expo(mods, S, S["E"], use_mask, use_depth)
    torch.cuda.synchronize()
    ref = _reference(S, S["E"].cpu(), use_mask, use_depth)
    want = ref["dE"].reshape(12)
    rel = float((dE.cpu().double() - want).norm() / want.norm())
    dl = abs(float(loss) - ref["loss"])
    print(f"exposure fused {IDS[CASES.index((W, H, n, use_mask, use_depth, bg, shift))]}: dE relL2 {rel:.2e} (bar {GRAD_TOL:.0e}); "
          f"loss {float(loss):.7f} float64 {ref['loss']:.7f} diff {dl:.2e}; margin {ref['margin']:.2e}")
    assert ref["margin"] > 1e-4  # no value near a kink: a float32 evaluation has every sign right
    assert float(want.norm()) > 0.0 and rel <= GRAD_TOL
    assert dl <= 1e-6 * max(1.0, abs(ref["loss"]))
    if shift:
        assert not sums.any()  # a view without pairs: its loss and d E are the background's, its sums zero


# ---- 3. the Gaussians' gradients against the composed chain --------------------------------------------------------------
def _composed(mods, S, E, use_mask, use_depth):
    """(unscaled loss, gradients) of forward image -> exposed colour and loss in torch -> autograd -> gr_bwd."""
    tr, _, losses, _ = mods
    pred = S["out"].clone().requires_grad_(True)
    a = S["alpha"].clone().requires_grad_(True)
    d = S["depth"].clone().requires_grad_(True) if use_depth else None
    y = pred
    if E is not None:
        # Channel by channel in element-wise operations, so that the order in which autograd adds the three terms
        # E[k][j] g_k of d / d out_j is defined: the engine runs later-built nodes first, so with the rows built 2, 1, 0
        # it adds k = 0, 1, 2, the order the kernel states ((E[0][j] g_0 + E[1][j] g_1) + E[2][j] g_2).  As the
        # broadcast expression y = out[..., 0:1] * E[:, 0] + ... the same gradient goes through a reduction kernel
        # whose summation order depends on the shape: on an MI355X it equals the stated order in every value at
        # 50 x 37 and differs by one ulp in 253 of 768 values at 16 x 16, and the two-piece bf16 operand split of the
        # backward splat turns that ulp into up to 4e-6 max|g| (measured: 4.7e-9 on d_scales), above the 1e-6 bound,
        # while gr_bwd on the stated order's upstream equals the entry bit for bit in all three shapes.
        x = [pred[..., j] for j in range(3)]
        rows = {k: ((x[0] * E[k, 0] + x[1] * E[k, 1]) + x[2] * E[k, 2]) + E[k, 3] for k in (2, 1, 0)}
        y = torch.stack([rows[0], rows[1], rows[2]], dim=-1)
    val = losses.l1_loss(y, S["target"])
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


@pytest.mark.parametrize("W,H,n,use_mask,use_depth,bg,shift", CASES[:6], ids=IDS[:6])
def test_matches_composed_chain(mods, cuda, W, H, n, use_mask, use_depth, bg, shift):
    tr = mods[0]
    S = _state(mods, cuda, W, H, n, use_depth, bg, shift)
    assert S["st"].num_pairs > 0
    mask = S["mask"] if use_mask else None
    td, wd = (S["tdepth"], W_DEPTH) if use_depth else (None, 0.0)
    # b0: identity E, the existing gr_bwd_fit against the composed chain without exposure (both older code)
    _, g0 = _composed(mods, S, None, use_mask, use_depth)
    f0 = tuple(torch.empty_like(t) for t in S["p"])
    tr.backward_fit_native(*S["p"], S["st"], S["target"], mask, W_SIL, td, wd, G_SCALE, torch.zeros(1, device=cuda), f0, False)
    base = [float((a - b).abs().max()) for a, b in zip(f0, g0)]
    val, gc = _composed(mods, S, S["E"], use_mask, use_depth)
    loss, _, sums, sums3 = _expo(mods, S, S["E"], use_mask, use_depth)
    gf = tuple(torch.empty_like(t) for t in S["p"])
    tr.reduce_sums_native(*S["p"], [(S["st"].gv, sums, sums3) if use_depth else (S["st"].gv, sums)], gf, accumulate=False)
    torch.cuda.synchronize()
    dl = abs(float(loss) - val)
    print(f"exposure fused {W}x{H}: loss {float(loss):.7f} composed {val:.7f} diff {dl:.2e}")
    ok = dl <= 1e-6 * max(1.0, abs(val))
    for name, a, b, b0 in zip(NAMES, gf, gc, base):
        d, gmax = float((a - b).abs().max()), float(b.abs().max())
        bound = max(4.0 * b0, 1e-6 * gmax)
        print(f"  {name}: diff {d:.3e} (identity, gr_bwd_fit: {b0:.3e}) max|g| {gmax:.3e} bound {bound:.3e}")
        assert torch.isfinite(a).all()
        ok = ok and d <= bound
    assert ok and float(gc[0].abs().max()) > 0.0  # (a 7 x 5 view clamps every sigma: its scale gradients are zero)


# ---- 4. determinism -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_depth", [False, True])
def test_two_calls_are_equal(mods, cuda, use_depth):
    S = _state(mods, cuda, 50, 37, 1500, use_depth)
    a = _expo(mods, S, S["E"], True, use_depth)
    b = _expo(mods, S, S["E"], True, use_depth)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert (x is None and y is None) or torch.equal(x, y)


# ---- 5. refusals --------------------------------------------------------------------------------------------------------
def test_errors(mods, cuda):
    tr = mods[0]
    nat = tr._native
    L = nat.lib()
    S = _state(mods, cuda, 50, 37, 1500)
    st = S["st"]
    need = int(L.gr_bwd_exposure_bytes(ctypes.byref(st.gv), st.n, ctypes.byref(st.plan)))
    tiles = -(-50 // 16) * -(-37 // 16)
    assert need >= int(L.gr_bwd_bytes(ctypes.byref(st.gv), st.n, ctypes.byref(st.plan))) + 48 * tiles
    ws = torch.zeros((need,), dtype=torch.uint8, device=cuda)
    loss = torch.zeros(1, device=cuda)
    sums = torch.zeros((st.n, 8), device=cuda)
    dE = torch.zeros(12, device=cuda)
    stream = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)

    def call(gv, E, d_E, ws_bytes):
        return L.gr_bwd_fit_exposure_gather(ctypes.byref(gv), st.n, ctypes.byref(st.plan), nat.ptr(st.geom), nat.ptr(st.bins),
                                            nat.ptr(st.saved), nat.ptr(S["target"]), nat.ptr(S["mask"]), ctypes.c_float(W_SIL),
                                            None, ctypes.c_float(0.0), ctypes.c_float(G_SCALE), E, d_E, nat.ptr(loss),
                                            nat.ptr(ws), ws_bytes, nat.ptr(sums), None, stream)

    E = nat.ptr(S["E"])
    assert call(st.gv, None, nat.ptr(dE), need) == nat.GR_ERR_INVALID_ARGUMENT and b"exposure is null" in L.gr_last_error()
    assert call(st.gv, E, None, need) == nat.GR_ERR_INVALID_ARGUMENT and b"d_exposure is null" in L.gr_last_error()
    assert call(st.gv, E, nat.ptr(dE), need - 1) == nat.GR_ERR_WORKSPACE and b"workspace" in L.gr_last_error()
    t32 = nat.GrView.from_buffer_copy(st.gv)
    t32.tile = 32
    assert call(t32, E, nat.ptr(dE), need) == nat.GR_ERR_INVALID_ARGUMENT and b"32-pixel" in L.gr_last_error()
    band = nat.GrView.from_buffer_copy(st.gv)
    band.row0, band.rows = 0, 1
    assert call(band, E, nat.ptr(dE), need) == nat.GR_ERR_INVALID_ARGUMENT and b"band" in L.gr_last_error()
    for bad in (S["E"].reshape(12)[:11], S["E"].double(), S["E"].cpu(), torch.zeros((12, 2), device=cuda)[:, 0]):
        with pytest.raises(ValueError, match="exposure"):
            tr.backward_fit_exposure_gather_native(st, S["target"], S["mask"], W_SIL, None, 0.0, G_SCALE, bad, dE, loss)
        with pytest.raises(ValueError, match="d_exposure"):
            tr.backward_fit_exposure_gather_native(st, S["target"], S["mask"], W_SIL, None, 0.0, G_SCALE, S["E"], bad, loss)
    torch.cuda.synchronize()
    assert not sums.any() and not dE.any() and float(loss) == 0.0  # a rejected call launches nothing


# ---- 6. the fitter ------------------------------------------------------------------------------------------------------
FW, FH, FN, FV = 64, 48, 300, 6


@pytest.fixture()
def python_schedule(mods):
    """The Python schedule, eagerly: no captured / batched step and no native executor (neither has an exposure form;
    the fitters compared with an exposure fit run the same schedule)."""
    fm = mods[1]
    saved = fm.GRAPH_MODE, fm.NATIVE_EXEC
    fm.GRAPH_MODE, fm.NATIVE_EXEC = "0", "0"
    yield fm
    fm.GRAPH_MODE, fm.NATIVE_EXEC = saved


def _fit_scene(fm, cuda, depths=False):
    cams = fm.orbit_cameras(FV, FW, FH, cuda)
    g = torch.Generator(device=cuda).manual_seed(21)
    targets = [torch.rand((FH, FW, 3), generator=g, device=cuda) for _ in range(FV)]
    masks = [(t.mean(dim=2) > 0.5).float() for t in targets]
    dep = [torch.rand((FH, FW), generator=g, device=cuda) for _ in range(FV)] if depths else None
    return cams, targets, masks, dep


def test_fitter_identity_on_fixed_views_is_the_depth_form(mods, cuda, python_schedule):
    fm, bench = python_schedule, mods[3]
    cams, targets, masks, depths = _fit_scene(fm, cuda, depths=True)
    runs = []
    for kw in ({}, {"exposure": True, "exposure_fused": True, "exposure_fixed": tuple(range(FV))}):
        f = fm.ViewShardedFitter(bench.synthetic_params(FN, cuda), cams, targets, FW, FH, masks=masks, depths=depths, **kw)
        assert f._form() == ("exposure" if kw else "depth")
        losses = [f.step().clone() for _ in range(3)]
        runs.append((losses, {k: v.detach().clone() for k, v in f.params.items()}, f))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
    assert all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1])
    E, dE = runs[1][2].exposure_state()
    assert all(torch.equal(E[v], EYE) for v in range(FV)) and not dE.any()


def test_fitter_gradient_matches_the_dense_reference(mods, cuda, python_schedule):
    """One step from identity on the recovery scene (signed exposures: every residual at least 0.02 from zero, so the
    HIP render and the dense one take the same signs): d loss / d E of the free views against dense_sums + view_loss,
    within 4 x the HIP render's own distance from the dense image (d E is linear in the render)."""
    tr, fm = mods[0], python_schedule
    V, W, H = eref.V, eref.W, eref.H
    fit, E_true = eref.recovery_fitter(fm, cuda, signed=True, exposure_fused=True)
    assert fit._form() == "exposure"
    scene = eref.scene_arrays(5)
    cams = orc.orbit_cameras(V, W, H)
    m, s, c, o = (t.detach().contiguous() for t in fm.activations(fit.params))
    want, num, den = [], 0.0, 0.0
    for i in range(1, V):
        sums = eref.dense_sums(*scene, *cams[i], W, H)
        want.append(eref.view_loss(sums, None, EYE, fit.targets[i], g_scale=1.0 / V)["dE"])
        dense = eref.exposed(sums, None, EYE)[1]
        out = tr.forward_native(m, s, c, o, fit._gr_view("ssim", i, cuda))[0]
        num += float((out.cpu().double() - dense).pow(2).sum())
        den += float(dense.pow(2).sum())
    d0 = (num / den) ** 0.5
    fit.step()
    E1, dE = fit.exposure_state()
    want = torch.stack(want)
    rel = float((dE[1:].double() - want).norm() / want.norm())
    print(f"fitter d loss / d E vs the dense float64 reference: relL2 {rel:.2e}; the HIP render vs the dense image: d0 {d0:.2e}; "
          f"bound {max(4.0 * d0, 1e-6):.2e}")
    assert float(want.norm()) > 0.0 and rel <= max(4.0 * d0, 1e-6)
    # (d) the fixed row keeps E and reports a zero gradient; the free rows moved by Adam's first step
    assert torch.equal(E1[0], EYE) and not dE[0].any()
    assert torch.allclose(E1[1:], EYE - 5e-3 * dE[1:] / (dE[1:].abs() + 1e-8), rtol=0, atol=5e-7)


def test_fitter_recovery(mods, cuda, python_schedule):
    fm = python_schedule
    fit, E_true = eref.recovery_fitter(fm, cuda, exposure_fused=True)
    e0 = eref.exposure_error(fit.exposure_state()[0], E_true)
    before = {k: v.detach().clone() for k, v in fit.params.items()}
    for _ in range(eref.RECOVERY_STEPS):
        fit.step()
    E, dE = fit.exposure_state()
    e1 = eref.exposure_error(E, E_true)
    print(f"HIP device: mean |E - E_true| {e0:.5f} -> {e1:.5f} (ratio {e1 / e0:.3f}) after {eref.RECOVERY_STEPS} steps")
    assert all(torch.equal(before[k], fit.params[k].detach()) for k in before)  # lr = 0: the Gaussians stay exact
    assert torch.equal(E[0], E_true[0]) and not dE[0].any()  # the fixed view
    assert e1 <= 0.5 * e0


@pytest.mark.parametrize("extra", ["refine_cameras", "density_stats"])
def test_fitter_beside_the_other_extensions(mods, cuda, python_schedule, extra):
    fm, bench = python_schedule, mods[3]
    cams, targets, masks, _ = _fit_scene(fm, cuda)
    f = fm.ViewShardedFitter(bench.synthetic_params(FN, cuda), cams, targets, FW, FH, masks=masks, exposure=True,
                             exposure_fused=True, **{extra: True})
    loss = f.step()
    E, dE = f.exposure_state()
    assert torch.isfinite(loss) and torch.isfinite(E).all() and torch.isfinite(dE).all() and float(dE[1:].abs().max()) > 0.0
    assert all(torch.isfinite(p).all() for p in f.params.values())
    if extra == "refine_cameras":
        xi, dxi = f.camera_state()
        assert torch.isfinite(xi).all() and torch.isfinite(dxi).all() and float(dxi.abs().max()) > 0.0
    else:
        gsum, seen = f.density_state()
        assert torch.isfinite(gsum).all() and float(gsum.max()) > 0.0 and float(seen.max()) > 0.0
