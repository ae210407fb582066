"""GPU: per-pixel loss weights on the HIP device.  Kernel level: gr_bwd_fit_weighted_gather (k_pixel_grads_wgt and
k_depth_tile_sums_wgt in libgr_hip.so) against gr_bwd_fit_gather at weights of ones (bit for bit) and at weights of two
(2 g_scale, bit for bit), zero-weight independence, the loss against the float64 restatement tests/weights_reference.py
on the kernel's own saved sums, the Gaussians' gradients against the chain composed from the older entries (forward image
-> weighted loss in torch -> autograd -> gr_bwd), determinism and the arrival ticket.  Fitter level:
ViewShardedFitter(weights=...) on the Python schedule against the depth form (ones), against the host fitter, refusals.

The figures the tests print on an MI355X are recorded in DESIGN.md section 8p and profiles/weights.txt.
"""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import pytest
import torch

from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import exposure_reference as eref  # noqa: E402
import handoff_reference as hr  # noqa: E402
import weights_reference as wref  # noqa: E402

pytestmark = pytest.mark.gpu

W_SIL, W_DEPTH, G_SCALE = 0.2, 0.05, 0.25
NAMES = ("d_means", "d_scales", "d_colors", "d_opacities")
RECTS = wref.GPU_RECTS  # the zero rectangle per view size (tests/test_weights_cpu.py checks what each covers)


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


def _state(mods, cuda, W, H, n, depth=False, bg=None, shift=0.0):
    """One view of n Gaussians rendered once (shared by the tests, left unchanged): parameters, forward, targets and
    depth target kept 1e-3 from the kinks of the L1 terms (against float64 images of the kernel's own saved sums), the
    weight map and a second set of targets that differs inside the zero rectangle only."""
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
        target = torch.rand((H, W, 3), generator=g)
        mask = (torch.rand((H, W), generator=g) > 0.5).float()
        tdepth = torch.rand((H, W), generator=g)
        gv = tr.make_view(cam.view, cam.proj, W, H, list(bg) if bg else None, depth_grad=depth)
        out, alpha, dimg, st = tr.forward_native(m, s, c, o, gv)
        torch.cuda.synchronize()
        sums = _host_sums(st, W, H)
        bgt = None if bg is None else torch.tensor(bg)
        out64, _, depth64 = eref.exposed(sums, bgt, torch.eye(3, 4))[1:]
        dn64 = depth64 / (depth64.max() + 1e-6)
        for _ in range(3):  # (a value pushed off one kink may land by another: a second and third pass)
            target = wref.clear_targets(out64, target)
            tdepth = wref.clear_targets(dn64, tdepth)
        assert float((out64 - target.double()).abs().min()) >= 0.9e-3 and float((dn64 - tdepth.double()).abs().min()) >= 0.9e-3
        rect = RECTS[(W, H)]
        x0, y0, x1, y1 = rect
        weight = wref.weight_map(W, H, rect, wref.GPU_WEIGHT_SEED)
        other = dict(target=target.clone(), mask=mask.clone(), tdepth=tdepth.clone())
        other["target"][y0:y1, x0:x1] = 1.0 - target[y0:y1, x0:x1]
        other["mask"][y0:y1, x0:x1] = 1.0 - mask[y0:y1, x0:x1]
        other["tdepth"][y0:y1, x0:x1] = 0.5 * tdepth[y0:y1, x0:x1] + 0.3
        _STATES[key] = dict(p=(m, s, c, o), target=target.to(cuda), mask=mask.to(cuda), tdepth=tdepth.to(cuda), out=out,
                            alpha=alpha, depth=dimg, st=st, sums=sums, bg=bgt, W=W, H=H, weight=weight.to(cuda),
                            other={k: v.to(cuda) for k, v in other.items()})
    return _STATES[key]


def _plain(mods, S, use_mask, use_depth, g_scale=G_SCALE):
    """gr_bwd_fit_gather on the state: (loss, sums, sums3)."""
    loss = torch.zeros(1, device=S["out"].device)
    sums, sums3 = mods[0].backward_fit_gather_native(S["st"], S["target"], S["mask"] if use_mask else None, W_SIL,
                                                     S["tdepth"] if use_depth else None, W_DEPTH if use_depth else 0.0,
                                                     g_scale, loss)
    return loss, sums, sums3


def _weighted(mods, S, weight, use_mask, use_depth, g_scale=G_SCALE, src=None):
    """gr_bwd_fit_weighted_gather on the state (targets from ``src``, default the state's): (loss, sums, sums3)."""
    src = S if src is None else src
    loss = torch.zeros(1, device=S["out"].device)
    sums, sums3 = mods[0].backward_fit_weighted_gather_native(
        S["st"], src["target"], src["mask"] if use_mask else None, W_SIL, src["tdepth"] if use_depth else None,
        W_DEPTH if use_depth else 0.0, g_scale, weight, loss)
    return loss, sums, sums3


CASES = [
    # W, H, n, mask, depth, background, shift
    (50, 37, 1500, True, False, None, 0.0),   # partial tiles on both edges, 12 tiles: the fan-in crosses blocks
    (50, 37, 1500, False, False, None, 0.0),
    (50, 37, 1500, True, True, None, 0.0),    # a depth target (no_depth_grad = 0)
    (50, 37, 1500, False, True, None, 0.0),
    (50, 37, 1500, True, False, (0.2, 0.5, 0.7), 0.0),
    (16, 16, 400, True, False, None, 0.0),    # exactly one tile: the elected block is the only one
    (16, 16, 400, True, True, None, 0.0),
    (7, 5, 200, True, False, None, 0.0),      # smaller than a tile
    (7, 5, 200, False, True, None, 0.0),
    (50, 37, 300, True, False, (0.2, 0.5, 0.7), 1000.0),  # out of sight: num_pairs == 0
]
IDS = [f"{c[0]}x{c[1]}{'-mask' if c[3] else ''}{'-depth' if c[4] else ''}{'-bg' if c[5] else ''}{'-nopairs' if c[6] else ''}"
       for c in CASES]
WITH_PAIRS = [c for c in CASES if not c[6]]


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


# ---- 1. ones are today's entry, bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,n,use_mask,use_depth,bg,shift", CASES, ids=IDS)
def test_ones_are_gr_bwd_fit_gather(mods, cuda, W, H, n, use_mask, use_depth, bg, shift):
    S = _state(mods, cuda, W, H, n, use_depth, bg, shift)
    assert (S["st"].num_pairs == 0) == (shift != 0.0)
    la, sa, sa3 = _plain(mods, S, use_mask, use_depth)
    lb, sb, sb3 = _weighted(mods, S, torch.ones((H, W), device=cuda), use_mask, use_depth)
    torch.cuda.synchronize()
    assert float(la) > 0.0 and torch.equal(la, lb) and torch.equal(sa, sb)
    assert (sb3 is not None) == use_depth
    if use_depth:
        assert torch.equal(sa3, sb3)
    else:
        assert not sa3.any()
    assert bool(sb.any()) == (shift == 0.0)  # a view without pairs: its loss is the background's, its sums zero


# ---- 2. a power of two: every term carries the weight, the max's chain term included --------------------------------------
@pytest.mark.parametrize("W,H,n,use_mask", [(50, 37, 1500, True), (50, 37, 1500, False), (16, 16, 400, True), (7, 5, 200, True)])
def test_twos_are_twice_g_scale(mods, cuda, W, H, n, use_mask):
    S = _state(mods, cuda, W, H, n, True)
    one, two = torch.ones((H, W), device=cuda), torch.full((H, W), 2.0, device=cuda)
    la, sa, sa3 = _weighted(mods, S, one, use_mask, True, g_scale=2.0 * G_SCALE)
    lb, sb, sb3 = _weighted(mods, S, two, use_mask, True)
    l1, s1, s13 = _weighted(mods, S, one, use_mask, True)
    torch.cuda.synchronize()
    assert sa.any() and sa3.any() and torch.equal(sa, sb) and torch.equal(sa3, sb3)
    assert torch.equal(la, l1) and float(lb) == 2.0 * float(l1) and float(l1) > 0.0  # (the loss is not scaled by g_scale)
    assert not torch.equal(s1, sb) and not torch.equal(s13, sb3)


# ---- 3. a zero weight hides the pixel's targets ----------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,n,use_mask,use_depth,bg,shift", CASES, ids=IDS)
def test_zero_weight_independence(mods, cuda, W, H, n, use_mask, use_depth, bg, shift):
    S = _state(mods, cuda, W, H, n, use_depth, bg, shift)
    a = _weighted(mods, S, S["weight"], use_mask, use_depth)
    b = _weighted(mods, S, S["weight"], use_mask, use_depth, src=S["other"])
    c = _weighted(mods, S, torch.ones((H, W), device=cuda), use_mask, use_depth, src=S["other"])
    one = _weighted(mods, S, torch.ones((H, W), device=cuda), use_mask, use_depth)
    torch.cuda.synchronize()
    assert _same(a, b)
    assert not torch.equal(c[0], one[0])  # (seen, the other targets do change the result)
    if not shift:
        assert not torch.equal(c[1], one[1]) and not torch.equal(a[1], one[1])


# ---- 4. random weights: the loss against float64, the gradients against the composed chain -----------------------------------
def _reduce(mods, S, sums, sums3, use_depth):
    gf = tuple(torch.empty_like(t) for t in S["p"])
    mods[0].reduce_sums_native(*S["p"], [(S["st"].gv, sums, sums3) if use_depth else (S["st"].gv, sums)], gf, accumulate=False)
    return gf


def _composed_plain(mods, S, use_mask, use_depth):
    """(unscaled loss, gradients) of forward image -> loss in torch -> autograd -> gr_bwd, without weights (the chain
    tests/test_exposure_fused_gpu.py composes at identity exposure)."""
    tr, _, losses, _ = mods
    pred = S["out"].clone().requires_grad_(True)
    a = S["alpha"].clone().requires_grad_(True)
    d = S["depth"].clone().requires_grad_(True) if use_depth else None
    val = losses.l1_loss(pred, S["target"])
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


def _composed_weighted(mods, S, use_mask, use_depth):
    """The same chain with the weighted loss.  Each term is written as sum_p |.| (w_p c) with c the term's float32
    constant (g_scale / (3 HW), w_sil g_scale / HW, w_depth g_scale / HW, each product and quotient rounded to float32
    as the kernel forms it), so autograd hands gr_bwd sign(.) round(w_p c) per value, the product the kernel states
    ((sign c) w; a product with a sign is exact): written as G_SCALE x mean(w |.|), the constant would reach the
    gradient through torch's division by an element count, a product with the rounded reciprocal."""
    tr = mods[0]
    f = np.float32
    HW = f(S["W"]) * f(S["H"])
    c_rgb = float(f(G_SCALE) / (f(3.0) * HW))
    c_sil = float((f(W_SIL) * f(G_SCALE)) / HW)
    c_dep = float((f(W_DEPTH) * f(G_SCALE)) / HW)
    w = S["weight"]
    pred = S["out"].clone().requires_grad_(True)
    a = S["alpha"].clone().requires_grad_(True)
    d = S["depth"].clone().requires_grad_(True) if use_depth else None
    scaled = (torch.abs(pred - S["target"]) * (w * c_rgb)[..., None]).sum()
    val = torch.mean(w[..., None] * torch.abs(pred.detach() - S["target"]))
    if use_mask:
        scaled = scaled + (torch.abs(a - S["mask"]) * (w * c_sil)).sum()
        val = val + W_SIL * torch.mean(w * torch.abs(a.detach() - S["mask"]))
    if use_depth:
        scaled = scaled + (torch.abs(d / (d.max() + 1e-6) - S["tdepth"]) * (w * c_dep)).sum()
        val = val + W_DEPTH * torch.mean(w * torch.abs(d.detach() / (d.detach().max() + 1e-6) - S["tdepth"]))
    ins = [pred] + ([a] if use_mask else []) + ([d] if use_depth else [])
    gs = list(torch.autograd.grad(scaled, ins))
    g_rgb = gs.pop(0).contiguous()
    g_alpha = gs.pop(0).contiguous() if use_mask else None
    g_depth = gs.pop(0).contiguous() if use_depth else None
    return float(val), tr.backward_native(*S["p"], S["st"], g_rgb, g_alpha, g_depth)


@pytest.mark.parametrize("W,H,n,use_mask,use_depth,bg,shift", CASES, ids=IDS)
def test_loss_matches_float64(mods, cuda, W, H, n, use_mask, use_depth, bg, shift):
    S = _state(mods, cuda, W, H, n, use_depth, bg, shift)
    loss, sums, _ = _weighted(mods, S, S["weight"], use_mask, use_depth)
    torch.cuda.synchronize()
    ref = wref.view_loss(S["sums"], S["bg"], S["weight"], S["target"], S["mask"] if use_mask else None, W_SIL,
                         S["tdepth"] if use_depth else None, W_DEPTH, G_SCALE)
    dl = abs(float(loss) - ref["loss"])
    print(f"weighted {IDS[CASES.index((W, H, n, use_mask, use_depth, bg, shift))]}: loss {float(loss):.7f} float64 "
          f"{ref['loss']:.7f} diff {dl:.2e} (bar 1e-6); margin {ref['margin']:.2e}")
    assert ref["margin"] > 1e-4 and ref["loss"] > 0.0
    assert dl <= 1e-6 * max(1.0, abs(ref["loss"]))
    if shift:
        assert not sums.any()


@pytest.mark.parametrize("W,H,n,use_mask,use_depth,bg,shift", WITH_PAIRS, ids=IDS[:len(WITH_PAIRS)])
def test_matches_composed_chain(mods, cuda, W, H, n, use_mask, use_depth, bg, shift):
    """Bound: DESIGN.md section 8g's rule as tests/test_exposure_fused_gpu.py states it, max(4 b0, 1e-6 max|g|) with b0 the
    distance gr_bwd_fit_gather (the same inputs, no weights) has from its own composed chain, measured here: the yardstick
    is the existing form, not the code under test.

    Measured on an MI355X: every tensor equal bit for bit in every case (b0 = 0 without a depth term; 3.2e-9 / 8.4e-9 /
    0 / 1.3e-9 with one at 50 x 37, where the weighted entry still equals its chain), except with a depth term at
    16 x 16 (d_means 1.2e-10, d_scales 1.2e-10, d_opacities 3.8e-10 at max|g| 2.4e-3 / 4.6e-3 / 3.5e-3, b0 = 0 there) and
    at 7 x 5 (8.7e-11 / 0 / 0 / 2.3e-10 beside b0 4.4e-11 / 0 / 0 / 1.2e-10).  The 16 x 16 case passes by the rule's second
    term only (1.1e-7 max|g|): 4 b0 alone would ask for equal bits there.  What differs is one value of the upstream
    depth gradient, the arg-max pixel's, by one ulp (2.3e-10 at 3.6e-3): its share of the max's gradient is a float32
    reduction over the pixels in the chain and a double sum in the kernel (depth_final).  The chain without weights
    differs from the kernel's arithmetic in that value too; there the ulp is lost in the splat's float32 sums."""
    S = _state(mods, cuda, W, H, n, use_depth, bg, shift)
    assert S["st"].num_pairs > 0
    _, g0 = _composed_plain(mods, S, use_mask, use_depth)
    _, s0, s03 = _plain(mods, S, use_mask, use_depth)
    f0 = _reduce(mods, S, s0, s03, use_depth)
    base = [float((a - b).abs().max()) for a, b in zip(f0, g0)]
    val, gc = _composed_weighted(mods, S, use_mask, use_depth)
    loss, sums, sums3 = _weighted(mods, S, S["weight"], use_mask, use_depth)
    gf = _reduce(mods, S, sums, sums3, use_depth)
    torch.cuda.synchronize()
    dl = abs(float(loss) - val)
    print(f"weighted {W}x{H}{' mask' if use_mask else ''}{' depth' if use_depth else ''}{' bg' if bg else ''}: loss "
          f"{float(loss):.7f} composed {val:.7f} diff {dl:.2e}")
    ok = dl <= 1e-6 * max(1.0, abs(val))
    for name, a, b, b0 in zip(NAMES, gf, gc, base):
        d, gmax = float((a - b).abs().max()), float(b.abs().max())
        bound = max(4.0 * b0, 1e-6 * gmax)
        print(f"  {name}: diff {d:.3e} (no weights, gr_bwd_fit_gather: {b0:.3e}) max|g| {gmax:.3e} bound {bound:.3e}")
        assert torch.isfinite(a).all()
        ok = ok and d <= bound
    assert ok and float(gc[0].abs().max()) > 0.0  # (a 7 x 5 view clamps every sigma: its scale gradients are zero)


# ---- 5. determinism, the ticket ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_depth", [False, True])
def test_two_calls_are_equal_and_the_ticket_is_left_zero(mods, cuda, use_depth):
    S = _state(mods, cuda, 50, 37, 1500, use_depth)
    nat = mods[0]._native
    a = _weighted(mods, S, S["weight"], True, use_depth)
    b = _weighted(mods, S, S["weight"], True, use_depth)
    torch.cuda.synchronize()
    assert _same(a, b)
    st = S["st"]
    off, _ = nat.items_layout(st.gv, st.n, st.num_pairs)
    tiles = 4 * 3
    raw = st.bins.cpu().numpy()
    hr.assert_tickets_zero(raw[off[3]:off[3] + 4 * hr.ticket_words(tiles)].view(np.int32), tiles)


def test_wrapper_refusals_launch_nothing(mods, cuda):
    tr = mods[0]
    S = _state(mods, cuda, 50, 37, 1500)
    loss = torch.zeros(1, device=cuda)
    w = S["weight"]
    for bad in (w[:36], w.double(), w.cpu(), torch.ones((37, 100), device=cuda)[:, ::2], None):
        with pytest.raises(ValueError, match="weight"):
            tr.backward_fit_weighted_gather_native(S["st"], S["target"], S["mask"], W_SIL, None, 0.0, G_SCALE, bad, loss)
    torch.cuda.synchronize()
    assert float(loss) == 0.0


# ---- 6. the fitter -----------------------------------------------------------------------------------------------------
FW, FH, FN, FV = 64, 48, 300, 6


@pytest.fixture()
def python_schedule(mods):
    """The Python schedule, eagerly: no captured / batched step and no native executor (neither has a weighted form;
    the fitters compared with a weighted fit run the same schedule)."""
    fm = mods[1]
    saved = fm.GRAPH_MODE, fm.NATIVE_EXEC
    fm.GRAPH_MODE, fm.NATIVE_EXEC = "0", "0"
    yield fm
    fm.GRAPH_MODE, fm.NATIVE_EXEC = saved


def _fit_scene(fm, cuda):
    cams = fm.orbit_cameras(FV, FW, FH, cuda)
    g = torch.Generator(device=cuda).manual_seed(21)
    targets = [torch.rand((FH, FW, 3), generator=g, device=cuda) for _ in range(FV)]
    masks = [(t.mean(dim=2) > 0.5).float() for t in targets]
    dep = [torch.rand((FH, FW), generator=g, device=cuda) for _ in range(FV)]
    return cams, targets, masks, dep


def test_fitter_ones_are_the_depth_form(mods, cuda, python_schedule):
    fm, bench = python_schedule, mods[3]
    cams, targets, masks, depths = _fit_scene(fm, cuda)
    runs = []
    for kw in ({}, {"weights": [torch.ones((FH, FW)) for _ in range(FV)]}):
        f = fm.ViewShardedFitter(bench.synthetic_params(FN, cuda), cams, targets, FW, FH, masks=masks, depths=depths, **kw)
        assert f._form() == ("weighted" if kw else "depth")
        assert kw == {} or (all(w.is_cuda and w.dtype == torch.float32 for w in f.weights) and not f._graph_ok(cuda))
        losses = [f.step().clone() for _ in range(3)]
        runs.append((losses, {k: v.detach().clone() for k, v in f.params.items()}))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
    assert all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1])


def test_fitter_ones_are_the_l1_loss_without_a_depth_term(mods, cuda, python_schedule):
    """Without a depth term the weighted form renders 16-pixel tiles into saved sums where the L1 form evaluates the loss
    in the 32-pixel forward's epilogue: two renders of the same views, so the first step's loss agrees within the
    project's parity bar (1e-4, relative)."""
    fm, bench = python_schedule, mods[3]
    cams, targets, masks, _ = _fit_scene(fm, cuda)
    plain = fm.ViewShardedFitter(bench.synthetic_params(FN, cuda), cams, targets, FW, FH, masks=masks)
    ones = fm.ViewShardedFitter(bench.synthetic_params(FN, cuda), cams, targets, FW, FH, masks=masks,
                                weights=[torch.ones((FH, FW)) for _ in range(FV)])
    assert ones._form() == "weighted" and plain._form() == "l1"
    a, b = float(plain.step()), float(ones.step())
    print(f"first-step loss: L1 form {a:.7f}, weighted form at ones {b:.7f}")
    assert abs(a - b) <= 1e-4 * abs(a) and all(torch.isfinite(p).all() for p in ones.params.values())


def test_fitter_matches_the_host_fitter(mods, cuda, python_schedule):
    """One step (lr = 0) with a depth term on exposure_reference's scene, targets and depth targets 1e-3 from the kinks
    of the dense render: the loss and the gradient norm against the host fitter, within 4 x the HIP render's own
    distance from the dense float64 image, measured here."""
    tr, fm = mods[0], python_schedule
    V, W, H = eref.V, eref.W, eref.H
    scene = eref.scene_arrays(5)
    cams = orc.orbit_cameras(V, W, H)
    g = torch.Generator().manual_seed(4)
    targets, depths, dense = [], [], []
    for view, proj in cams:
        out, _, depth = eref.exposed(wref.dense_sums(*scene, view, proj, W, H), None, torch.eye(3, 4))[1:]
        dense.append(out)
        targets.append(wref.clear_targets(out, torch.rand((H, W, 3), generator=g)))
        depths.append(wref.clear_targets(depth / (depth.max() + 1e-6), torch.rand((H, W), generator=g)))
    weights = [wref.weight_map(W, H, (10, 6, 24, 18), i) for i in range(V)]
    res = {}
    for dev in (torch.device("cpu"), cuda):
        fc = [tr.Camera(view=torch.from_numpy(np.asarray(v, np.float32)).to(dev),
                        proj=torch.from_numpy(np.asarray(p, np.float32)).to(dev)) for v, p in cams]
        fit = fm.ViewShardedFitter(eref.exact_params(scene, dev), fc, [t.to(dev) for t in targets], W, H, lr=0.0, masks=None,
                                   depths=[d.to(dev) for d in depths], weights=weights)
        assert fit._form() == ("weighted" if dev.type == "cuda" else "depth")
        loss = float(fit.step())
        gn = float(sum(float(p.grad.double().pow(2).sum()) for p in fit.params.values()) ** 0.5)
        res[dev.type] = (loss, gn, fit)
    fit = res["cuda"][2]
    m, s, c, o = (t.detach().contiguous() for t in fm.activations(fit.params))
    num = den = 0.0
    for i in range(V):
        out = tr.forward_native(m, s, c, o, fit._gr_view("depth", i, cuda))[0]
        num += float((out.cpu().double() - dense[i]).pow(2).sum())
        den += float(dense[i].pow(2).sum())
    d0 = (num / den) ** 0.5
    bound = max(4.0 * d0, 1e-6)
    (la, ga, _), (lb, gb, _) = res["cpu"], res["cuda"]
    print(f"weighted fitter, HIP device vs host tensors: loss {lb:.7f} / {la:.7f} (rel {abs(la - lb) / la:.2e}); gradient norm "
          f"{gb:.6e} / {ga:.6e} (rel {abs(ga - gb) / ga:.2e}); the HIP render vs the dense image d0 {d0:.2e}; bound {bound:.2e}")
    assert ga > 0.0 and abs(la - lb) <= bound * abs(la) and abs(ga - gb) <= bound * ga


def test_fitter_refusals(mods, cuda, python_schedule):
    fm, bench = python_schedule, mods[3]
    cams, targets, masks, _ = _fit_scene(fm, cuda)
    ones = [torch.ones((FH, FW)) for _ in range(FV)]
    with pytest.raises(ValueError, match="weights with exposure_fused"):
        fm.ViewShardedFitter(bench.synthetic_params(FN, cuda), cams, targets, FW, FH, masks=masks, weights=ones, exposure=True,
                             exposure_fused=True)
    with pytest.raises(ValueError, match="weights with dssim_weight > 0"):
        fm.ViewShardedFitter(bench.synthetic_params(FN, cuda), cams, targets, FW, FH, masks=masks, weights=ones,
                             dssim_weight=0.2, dssim_fused=True)
    with pytest.raises(ValueError, match="the weighted form is the fused fit path's.*a custom render_fn"):
        fm.ViewShardedFitter(bench.synthetic_params(FN, cuda), cams, targets, FW, FH, masks=masks, weights=ones,
                             render_fn=lambda *a, **k: None)


@pytest.mark.parametrize("extra", ["refine_cameras", "density_stats"])
def test_fitter_beside_the_other_extensions(mods, cuda, python_schedule, extra):
    fm, bench = python_schedule, mods[3]
    cams, targets, masks, _ = _fit_scene(fm, cuda)
    w = [wref.weight_map(FW, FH, (20, 10, 44, 30), i) for i in range(FV)]
    f = fm.ViewShardedFitter(bench.synthetic_params(FN, cuda), cams, targets, FW, FH, masks=masks, weights=w, **{extra: True})
    loss = f.step()
    assert torch.isfinite(loss) and all(torch.isfinite(p).all() for p in f.params.values())
    if extra == "refine_cameras":
        xi, dxi = f.camera_state()
        assert torch.isfinite(xi).all() and torch.isfinite(dxi).all() and float(dxi.abs().max()) > 0.0
    else:
        gsum, seen = f.density_state()
        assert torch.isfinite(gsum).all() and float(gsum.max()) > 0.0 and float(seen.max()) > 0.0
