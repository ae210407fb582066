"""GPU: colour-corrected held-out metrics.  Kernel level: gr_cc_fit_view (k_cc_moments + k_cc_solve) and gr_eval_view_cc
(k_eval_view<true> + k_eval_final) on a forward_native state, against the float64 numpy restatement (tests/cc_reference.py)
run on the image the existing forward composes from the same state.
  transform   within 1e-5 of the reference: a hundred times the float32 rounding of an entry near 1, four orders above
              the 1e-9 by which the order of a float64 moment sum moves an entry (include/gr_hip.h)
  cc_ssim     bit for bit 1 - losses.dssim_loss(losses.apply_color_transform(image, E_device), target): the staged render
              is that image's bits, and the SSIM sums are the older kernel's
  cc_l1, mse  within ssim_reference.VALUE_TOL of a float64 evaluation of that image (tests/test_eval_gpu.py's bar)
Executor level: gr_eval_views_cc against per-view calls, bit for bit.  Fitter level: evaluate(color_correct=True), the
executor against the Python schedule, its plain keys against evaluate(), interleaved with the other render-only passes,
and a fit with such an evaluation in it against the same fit without."""
from __future__ import annotations

import ctypes
import importlib
import math

import numpy as np
import pytest
import torch

import cc_reference as cc
import ssim_reference as ref

pytestmark = pytest.mark.gpu

BG = (0.2, 0.5, 0.7)
E_TOL = 1e-5
FW, FH, FV, FN = 96, 80, 6, 5000  # the fitter tests' shape (tests/test_eval_gpu.py)
ROW = 18


@pytest.fixture(scope="module")
def mods(pkg, cuda):
    return (importlib.import_module("3dgaussian_amd.torch_renderer"), importlib.import_module("3dgaussian_amd.fit_multiview"),
            importlib.import_module("3dgaussian_amd.losses"), importlib.import_module("bench"))


_STATES: dict = {}


def _state(mods, cuda, W, H, n, bg=None, bg_dev=False, shift=0.0, grey=False):
    """One view of n Gaussians on the orbit camera rendered once with images (shared, left unchanged) and a random
    target; bg through gr_view.background, or with bg_dev through background_dev; grey: equal colour channels."""
    key = (W, H, n, bg, bg_dev, shift, grey)
    if key not in _STATES:
        tr, fm, _, bench = mods
        p = bench.synthetic_params(n, cuda)
        with torch.no_grad():
            p["colors_raw"].add_(1.5)  # visible colours
            if grey:
                p["colors_raw"].copy_(p["colors_raw"][:, :1].expand(-1, 3))
            p["means"].add_(torch.tensor([0.0, shift, 0.0], device=cuda))  # (shift: far above every camera's view)
        m, s, c, o = (t.detach().contiguous() for t in fm.activations(p))
        cam = fm.orbit_cameras(3, W, H, cuda)[1]
        target = torch.rand((H, W, 3), generator=torch.Generator().manual_seed(11)).to(cuda)
        bgt = torch.tensor(bg, dtype=torch.float32, device=cuda) if bg and bg_dev else None
        gv = tr.make_view(cam.view, cam.proj, W, H, bgt if bg_dev else (list(bg) if bg else None), depth_grad=False)
        out, _, _, st = tr.forward_native(m, s, c, o, gv)
        torch.cuda.synchronize()
        _STATES[key] = dict(p=(m, s, c, o), target=target, out=out, st=st, keep=bgt)
    return _STATES[key]


def _fit_and_metrics(mods, cuda, st, target):
    """(E, the corrected metrics) of the two per-view calls, into sentinel-filled outputs."""
    tr = mods[0]
    E = torch.full((12,), -7.0, device=cuda)
    got = torch.full((3,), -1.0, device=cuda)
    tr.cc_fit_view_native(st, target, E)
    tr.eval_view_cc_native(st, target, E, got)
    return E, got


def _check(mods, cuda, S, tag, target=None):
    losses = mods[2]
    out = S["out"]
    target = S["target"] if target is None else target
    E, got = _fit_and_metrics(mods, cuda, S["st"], target)
    want_E = cc.fit(out, target)
    err = float(np.abs(E.cpu().numpy().astype(np.float64).reshape(3, 4) - want_E).max())
    y = losses.apply_color_transform(out, E)
    want_ssim = 1.0 - losses.dssim_loss(y, target)
    d = y.double() - target.double()
    l1, mse = float(d.abs().mean()), float((d * d).mean())
    plain = torch.full((3,), -1.0, device=cuda)
    mods[0].eval_view_native(S["st"], target, plain)
    print(f"cc {tag}: |E - ref| {err:.2e}; cc_l1 {float(got[0]):.8f} (f64 {l1:.8f}) cc_mse {float(got[1]):.8f} (f64 {mse:.8f}) "
          f"cc_ssim {float(got[2]):.8f} (kernel {float(want_ssim):.8f}); plain mse {float(plain[1]):.8f}; E "
          f"{[round(x, 5) for x in E.tolist()]}")
    assert bool(torch.isfinite(E).all()) and err <= E_TOL
    assert torch.equal(got[2], want_ssim)
    assert abs(float(got[0]) - l1) <= ref.VALUE_TOL
    assert abs(float(got[1]) - mse) <= ref.VALUE_TOL
    assert float(got[1]) <= float(plain[1]) + ref.VALUE_TOL  # the identity is feasible: corrected never worse
    return E, got


CASES = [
    # W, H, n  (tests/test_eval_gpu.py's sizes)
    (50, 37, 1500),  # partial tiles on both edges, a tile with all eight neighbours
    (16, 16, 400),   # exactly one tile
    (17, 15, 400),   # one off the tile edge each way
    (15, 17, 400),
    (7, 5, 200),     # smaller than the tile and the window
    (1, 1, 50),      # the smallest image
]


@pytest.mark.parametrize("W,H,n", CASES, ids=[f"{c[0]}x{c[1]}" for c in CASES])
def test_kernels_match_the_reference(mods, cuda, W, H, n):
    S = _state(mods, cuda, W, H, n)
    assert S["st"].num_pairs > 0 or W * H == 1
    _check(mods, cuda, S, f"{W}x{H}")


def test_more_than_256_tiles(mods, cuda):
    """260x257: 17 x 17 = 289 tiles, partial ones on both edges: the stride-256 sums of k_cc_solve and k_eval_final take a
    second turn."""
    S = _state(mods, cuda, 260, 257, 2000)
    assert S["st"].num_pairs > 0
    _check(mods, cuda, S, "260x257")


@pytest.mark.parametrize("W,H,n", [(50, 37, 1500), (7, 5, 200)], ids=["50x37", "7x5"])
def test_identity_transform_is_gr_eval_view(mods, cuda, W, H, n):
    """E = [I | 0]: the rendered colours are clamped to [0, 1], so 1 x0 + 0 x1 + 0 x2 + 0 is exactly x0 and the corrected
    metrics are gr_eval_view's bit for bit."""
    S = _state(mods, cuda, W, H, n)
    want = torch.full((3,), -1.0, device=cuda)
    mods[0].eval_view_native(S["st"], S["target"], want)
    got = torch.full((3,), -2.0, device=cuda)
    mods[0].eval_view_cc_native(S["st"], S["target"], torch.eye(3, 4, device=cuda).reshape(12).contiguous(), got)
    print(f"identity {W}x{H}: {got.tolist()} against gr_eval_view {want.tolist()}")
    assert torch.equal(got, want) and bool(torch.isfinite(want).all())


@pytest.mark.parametrize("bg_dev", [False, True], ids=["background", "background_dev"])
def test_background(mods, cuda, bg_dev):
    S = _state(mods, cuda, 50, 37, 1500, BG, bg_dev)
    assert not torch.equal(S["out"], _state(mods, cuda, 50, 37, 1500)["out"])  # (the background shows)
    E, got = _check(mods, cuda, S, "50x37 " + ("background_dev" if bg_dev else "background"))
    E2, got2 = _fit_and_metrics(mods, cuda, _state(mods, cuda, 50, 37, 1500, BG, not bg_dev)["st"], S["target"])
    assert torch.equal(E, E2) and torch.equal(got, got2)  # both ways of passing it give the same colours


def test_view_without_pairs(mods, cuda):
    """Gaussians moved out of view: a render of one colour (moments of rank 1), held by the ridge."""
    S = _state(mods, cuda, 50, 37, 300, BG, shift=1000.0)
    assert S["st"].num_pairs == 0
    assert torch.equal(S["out"], torch.tensor(BG, device=cuda).expand(37, 50, 3))
    _check(mods, cuda, S, "50x37 no pairs")


def test_grey_scene(mods, cuda):
    """Equal colour channels: moments of rank 2."""
    S = _state(mods, cuda, 50, 37, 1500, grey=True)
    out = S["out"]
    assert torch.equal(out[..., 0], out[..., 1]) and torch.equal(out[..., 0], out[..., 2]) and float(out.std()) > 0.01
    _check(mods, cuda, S, "50x37 grey")


def test_target_equal_to_the_render(mods, cuda):
    S = _state(mods, cuda, 50, 37, 1500)
    E, got = _check(mods, cuda, S, "50x37 target = render", target=S["out"].clone())
    assert float((E.cpu().double().reshape(3, 4) - torch.from_numpy(cc.IDENTITY)).abs().max()) <= 1e-6
    l1, mse, ssim = (float(x) for x in got)
    assert l1 <= ref.VALUE_TOL and mse <= ref.VALUE_TOL and abs(ssim - 1.0) <= ref.VALUE_TOL


def test_a_known_gain_is_removed(mods, cuda):
    """The target is 0.8 render + 0.03: the plain error is large, the corrected one none."""
    S = _state(mods, cuda, 50, 37, 1500)
    E, got = _check(mods, cuda, S, "50x37 gain", target=(0.8 * S["out"] + 0.03).contiguous())
    assert float(got[1]) < 1e-8


def test_deterministic(mods, cuda):
    S = _state(mods, cuda, 50, 37, 1500)
    a = _fit_and_metrics(mods, cuda, S["st"], S["target"])
    b = _fit_and_metrics(mods, cuda, S["st"], S["target"])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert bool(torch.isfinite(a[0]).all()) and bool(torch.isfinite(a[1]).all())


def test_argument_checks_launch_nothing(mods, cuda):
    tr = mods[0]
    nat = tr._native
    L = nat.lib()
    S = _state(mods, cuda, 50, 37, 1500)
    st = S["st"]
    need = int(L.gr_cc_ws_bytes(ctypes.byref(st.gv)))
    need_eval = int(L.gr_eval_ws_bytes(ctypes.byref(st.gv)))
    assert need >= 22 * 8 * 12
    ws = torch.zeros((max(need, need_eval),), dtype=torch.uint8, device=cuda)
    E = torch.full((12,), -7.0, device=cuda)
    got = torch.full((3,), -1.0, device=cuda)
    stream = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)

    def fit(gv, saved=st.saved, target=S["target"], ridge=1e-6, out=E, wsp=ws, ws_bytes=need):
        return L.gr_cc_fit_view(ctypes.byref(gv), nat.ptr(saved), nat.ptr(target), ctypes.c_float(ridge), nat.ptr(out),
                                nat.ptr(wsp), ws_bytes, stream)

    def evalcc(gv, saved=st.saved, target=S["target"], tf=E, out=got, wsp=ws, ws_bytes=need_eval):
        return L.gr_eval_view_cc(ctypes.byref(gv), nat.ptr(saved), nat.ptr(target), nat.ptr(tf), nat.ptr(out), nat.ptr(wsp),
                                 ws_bytes, stream)

    t32 = nat.GrView.from_buffer_copy(st.gv)
    t32.tile = 32
    band = nat.GrView.from_buffer_copy(st.gv)
    band.row0, band.rows = 0, 1
    for call in (fit, evalcc):
        assert call(t32) == nat.GR_ERR_INVALID_ARGUMENT and call(band) == nat.GR_ERR_INVALID_ARGUMENT
        for kw in (dict(saved=None), dict(target=None), dict(out=None), dict(wsp=None)):
            assert call(st.gv, **kw) == nat.GR_ERR_INVALID_ARGUMENT
    assert evalcc(st.gv, tf=None) == nat.GR_ERR_INVALID_ARGUMENT
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert fit(st.gv, ridge=bad) == nat.GR_ERR_INVALID_ARGUMENT and b"ridge" in L.gr_last_error()
    assert fit(st.gv, ws_bytes=need - 1) == nat.GR_ERR_WORKSPACE and b"workspace" in L.gr_last_error()
    assert evalcc(st.gv, ws_bytes=need_eval - 1) == nat.GR_ERR_WORKSPACE
    with pytest.raises(ValueError):
        tr.cc_fit_view_native(st, S["target"][:-1], E)
    with pytest.raises(ValueError):
        tr.eval_view_cc_native(st, S["target"], E[:-1], got)
    torch.cuda.synchronize()
    assert bool((E == -7.0).all()) and bool((got == -1.0).all()) and not ws.any()  # a rejected call launches nothing
    assert fit(st.gv) == nat.GR_OK and evalcc(st.gv) == nat.GR_OK
    torch.cuda.synchronize()
    assert bool((E != -7.0).all()) and bool((got != -1.0).all()) and ws.any()


# ---- executor and fitter level ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(mods, cuda):
    fm = mods[1]
    cams = fm.orbit_cameras(FV, FW, FH, cuda)
    g = torch.Generator(device=cuda).manual_seed(9)
    targets = [torch.rand((FH, FW, 3), generator=g, device=cuda) for _ in cams]
    masks = [(t.mean(dim=2) > 0.5).float() for t in targets]
    return cams, targets, masks


@pytest.fixture(scope="module")
def per_view(mods, cuda, scene):
    """The six views' rows by per-view forward_native + eval_view_native, cc_fit_view_native, eval_view_cc_native calls
    (computed once, left unchanged)."""
    tr, fm, _, bench = mods
    cams, targets, _ = scene
    p = bench.synthetic_params(FN, cuda)
    m, s, c, o = (t.detach().contiguous() for t in fm.activations(p))
    gvs = [tr.make_view(cam.view, cam.proj, FW, FH, None, depth_grad=False) for cam in cams]
    out = torch.zeros((FV, ROW), device=cuda)
    for j, gv in enumerate(gvs):
        _, _, _, st = tr.forward_native(m, s, c, o, gv, images=False)
        tr.eval_view_native(st, targets[j], out[j, :3])
        tr.cc_fit_view_native(st, targets[j], out[j, 6:])
        tr.eval_view_cc_native(st, targets[j], out[j, 6:], out[j, 3:6])
    torch.cuda.synchronize()
    return (m, s, c, o), gvs, out


@pytest.mark.parametrize("streams", [1, 3])
def test_executor_matches_per_view_calls(mods, cuda, scene, per_view, streams):
    tr = mods[0]
    nat = tr._native
    assert nat.EVAL_CC_ROW == ROW
    (m, s, c, o), gvs, want = per_view
    _, targets, _ = scene
    arr = (nat.GrFitTarget * FV)()
    for j in range(FV):
        arr[j].view = gvs[j]
        arr[j].target_rgb = targets[j].data_ptr()
    side = [torch.cuda.Stream(cuda) for _ in range(streams - 1)]
    prep = torch.cuda.Stream(cuda)
    cfg = nat.GrFitConfig(streams, 6, 4, 1, 0, 0)  # (reduce_batch / reduce_tail are ignored)
    rs = (ctypes.c_void_p * max(1, streams - 1))(*[x.cuda_stream for x in side])
    cfg.render_streams = rs
    cfg.prep_stream = prep.cuda_stream
    cur = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    args = (nat.executor(cuda.index or 0), ctypes.byref(cfg), FV, arr, FN, nat.ptr(m), nat.ptr(s), nat.ptr(c), 3, nat.ptr(o))
    got = [torch.full((FV, ROW), -1.0, device=cuda) for _ in range(2)]
    for g in got:
        nat.check(nat.lib().gr_eval_views_cc(*args, ctypes.c_float(1e-6), nat.ptr(g), cur), "gr_eval_views_cc")
    plain = torch.full((FV, 3), -1.0, device=cuda)
    nat.check(nat.lib().gr_eval_views(*args, nat.ptr(plain), cur), "gr_eval_views")
    refused = torch.full((FV, ROW), -1.0, device=cuda)
    assert nat.lib().gr_eval_views_cc(*args, ctypes.c_float(0.0), nat.ptr(refused), cur) == nat.GR_ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    print(f"gr_eval_views_cc, {streams} streams: {got[0][:2].tolist()}")
    assert torch.equal(got[0], want) and torch.equal(got[1], want)
    assert torch.equal(got[0][:, :3], plain)  # row[0..2] is gr_eval_view's
    assert bool((refused == -1.0).all())
    assert bool(torch.isfinite(want).all()) and bool((want[:, 4] > 0).all())
    assert bool((want[:, 4] <= want[:, 1] + ref.VALUE_TOL).all())


def _with(fm, **kw):
    saved = {k: getattr(fm, k) for k in kw}
    for k, v in kw.items():
        setattr(fm, k, v)
    return saved


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_fitter_evaluate(mods, cuda, scene):
    """evaluate(color_correct=True): the executor against the Python schedule bit for bit, its plain keys evaluate()'s,
    the values against the reference on the image of the fitter's own activated parameters; interleaved with
    contribution_state() and error_state() (which share the executor's pass workspace) the same bits again."""
    tr, fm, losses, bench = mods
    cams, targets, masks = scene
    res = {}
    for native in ("1", "0"):
        saved = _with(fm, NATIVE_EXEC=native, NUM_STREAMS=3)
        try:
            f = fm.ViewShardedFitter(bench.synthetic_params(FN, cuda), cams, targets, FW, FH, masks=masks)
            f.step()
            plain = f.evaluate()
            res[native] = f.evaluate(color_correct=True)
            assert f._eval_native_ok(cuda, targets) and f._native_exec() == (native == "1")
            for k in plain:
                assert np.array_equal(np.asarray(plain[k]), np.asarray(res[native][k])), k
            peak, err = f.contribution_state(), f.error_state()
            _same(f.evaluate(color_correct=True), res[native])
            assert torch.equal(f.contribution_state(), peak) and torch.equal(f.error_state(), err)
            _same(f.evaluate(), plain)
        finally:
            _with(fm, **saved)
    _same(res["1"], res["0"])
    got = res["0"]
    assert got["cc_transform"].shape == (FV, 3, 4) and got["cc_transform"].dtype == np.float64
    with torch.no_grad():
        own = [t.detach().float().contiguous() for t in f._eval_activations(cuda)]  # (what evaluate() renders)
        for i, (cam, t) in enumerate(zip(cams, targets)):
            # the image of the saved sums evaluate() reads (a render without images; black background), composed as
            # write_pixel does: this scene's moments have eigenvalues near the ridge (printed), where one ulp in a
            # few pixels of the image moves E by 1e-4 (the render with images and depth differs from this one in its
            # last bits in most values, and moved E by 5e-4), so the reference needs the very bits
            _, _, _, rs = tr.forward_native(*own, f._eval_view(cam, cuda), images=False)
            sv = rs.saved[:FH * FW * 4].reshape(FH, FW, 4)
            img = (sv[..., 1:4] / (1.0 + sv[..., :1])).clamp(0.0, 1.0)
            E = got["cc_transform"][i]
            A, _ = cc.moments(img, t)
            print(f"view {i}: |E - ref| {np.abs(E - cc.fit(img, t)).max():.2e}, moment eigenvalues "
                  f"{np.linalg.eigvalsh(A / (FW * FH)).tolist()}")
            assert np.abs(E - cc.fit(img, t)).max() <= E_TOL
            y = losses.apply_color_transform(img, torch.from_numpy(E))
            assert got["cc_ssim"][i] == float(1.0 - losses.dssim_loss(y, t))
            d = y.double() - t.double()
            assert abs(got["cc_l1"][i] - float(d.abs().mean())) <= ref.VALUE_TOL
            assert abs(got["cc_mse"][i] - float((d * d).mean())) <= ref.VALUE_TOL
            assert got["cc_psnr"][i] == -10.0 * math.log10(got["cc_mse"][i])
            assert got["cc_mse"][i] <= got["mse"][i] + ref.VALUE_TOL
    for k in ("l1", "mse", "psnr", "ssim"):
        assert got["mean_cc_" + k] == float(got["cc_" + k].mean())
    print(f"evaluate(color_correct=True): PSNR {got['psnr'].tolist()} corrected {got['cc_psnr'].tolist()}")
    sub = f.evaluate([cams[4], cams[1]], [targets[4], targets[1]], color_correct=True)
    assert np.array_equal(sub["cc_transform"], got["cc_transform"][[4, 1]])
    for k in ("cc_l1", "cc_mse", "cc_psnr", "cc_ssim"):
        assert sub[k].tolist() == [got[k][4], got[k][1]]


@pytest.mark.parametrize("mode", ["eager", "graph"])
@pytest.mark.parametrize("native", ["1", "0"], ids=["executor", "python"])
def test_evaluation_does_not_change_the_fit(mods, cuda, scene, mode, native):
    """Three steps against one step, evaluate(color_correct=True), two steps: losses, parameters and Adam moments bit
    for bit; eager, and graph: the captured batched step."""
    _, fm, _, bench = mods
    cams, targets, masks = scene
    saved = _with(fm, NATIVE_EXEC=native, GRAPH_MODE="0" if mode == "eager" else "batchgraph")
    try:
        runs = []
        for evaluate in (False, True):
            f = fm.ViewShardedFitter(bench.synthetic_params(FN, cuda), cams, targets, FW, FH, masks=masks)
            losses = [f.step()]
            assert f._graph_ok(cuda) == (mode == "graph")
            if evaluate:
                grads = {k: v.grad.detach().clone() for k, v in f.params.items()}
                r = f.evaluate(color_correct=True)
                assert all(math.isfinite(r["mean_cc_" + k]) for k in ("l1", "mse", "psnr", "ssim"))
                f.graph_sync()
                for k, v in f.params.items():
                    assert torch.equal(v.grad, grads[k]), k
            losses += [f.step() for _ in range(2)]
            f.graph_sync()
            torch.cuda.synchronize()
            runs.append(([float(x) for x in losses], {k: v.detach().clone() for k, v in f.params.items()},
                         {k: (f.opt.state[v]["exp_avg"].clone(), f.opt.state[v]["exp_avg_sq"].clone()) for k, v in f.params.items()}))
    finally:
        _with(fm, **saved)
    a, b = runs
    assert a[0] == b[0], (a[0], b[0])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
        assert torch.equal(a[2][k][0], b[2][k][0]) and torch.equal(a[2][k][1], b[2][k][1]), k
