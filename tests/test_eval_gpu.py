"""GPU: held-out evaluation.  Kernel level: gr_eval_view (k_eval_view + k_eval_final) on a forward_native state against
the image the existing forward composes from the same state: the SSIM metric bit for bit 1 - losses.dssim_loss (both
older kernels), l1 and mse within ssim_reference.VALUE_TOL of a float64 evaluation (a float tree sum of at most 768
terms per tile is under 1e-6 relative, the tiles are summed in double).  Executor level: gr_eval_views against per-view
calls, bit for bit.  Fitter level: ViewShardedFitter.evaluate against losses.image_metrics of render_gaussians_torch, the
executor against the Python schedule, and a fit with an evaluation in it against the same fit without."""
from __future__ import annotations

import ctypes
import importlib
import math

import pytest
import torch

import ssim_reference as ref

pytestmark = pytest.mark.gpu

BG = (0.2, 0.5, 0.7)
FW, FH, FV, FN = 96, 80, 6, 5000  # the fitter tests' shape (tests/test_dssim_fused_fit_gpu.py)


@pytest.fixture(scope="module")
def mods(pkg, cuda):
    return (importlib.import_module("3dgaussian_amd.torch_renderer"), importlib.import_module("3dgaussian_amd.fit_multiview"),
            importlib.import_module("3dgaussian_amd.losses"), importlib.import_module("bench"))


_STATES: dict = {}


def _state(mods, cuda, W, H, n, bg=None, bg_dev=False, shift=0.0):
    """One view of n Gaussians on the orbit camera rendered once with images (shared, left unchanged) and a random
    target; bg through gr_view.background, or with bg_dev through background_dev."""
    key = (W, H, n, bg, bg_dev, shift)
    if key not in _STATES:
        tr, fm, _, bench = mods
        p = bench.synthetic_params(n, cuda)
        with torch.no_grad():
            p["colors_raw"].add_(1.5)  # visible colours
            p["means"].add_(torch.tensor([0.0, shift, 0.0], device=cuda))  # (shift: far above every camera's view)
        m, s, c, o = (t.detach().contiguous() for t in fm.activations(p))
        cam = fm.orbit_cameras(3, W, H, cuda)[1]
        target = torch.rand((H, W, 3), generator=torch.Generator().manual_seed(11)).to(cuda)
        bgt = torch.tensor(bg, dtype=torch.float32, device=cuda) if bg and bg_dev else None
        gv = tr.make_view(cam.view, cam.proj, W, H, bgt if bg_dev else (list(bg) if bg else None), depth_grad=False)
        assert bool(gv.background_dev) == bool(bg and bg_dev)
        out, _, _, st = tr.forward_native(m, s, c, o, gv)
        torch.cuda.synchronize()
        _STATES[key] = dict(p=(m, s, c, o), target=target, out=out, st=st, keep=bgt)
    return _STATES[key]


def _metrics(mods, cuda, st, target):
    got = torch.full((3,), -1.0, device=cuda)
    mods[0].eval_view_native(st, target, got)
    return got


def _check(mods, cuda, S, tag):
    losses = mods[2]
    out, target = S["out"], S["target"]
    got = _metrics(mods, cuda, S["st"], target)
    want_ssim = 1.0 - losses.dssim_loss(out, target)
    d = out.double() - target.double()
    l1, mse = float(d.abs().mean()), float((d * d).mean())
    dense = 1.0 - float(ref.dssim_dense(out.double().cpu(), target.double().cpu()))
    print(f"eval {tag}: l1 {float(got[0]):.8f} (f64 {l1:.8f}) mse {float(got[1]):.8f} (f64 {mse:.8f}) "
          f"ssim {float(got[2]):.8f} (kernel {float(want_ssim):.8f}, dense f64 {dense:.8f})")
    assert torch.equal(got[2], want_ssim)
    assert abs(float(got[0]) - l1) <= ref.VALUE_TOL
    assert abs(float(got[1]) - mse) <= ref.VALUE_TOL
    assert abs(float(got[2]) - dense) <= ref.VALUE_TOL
    return got


CASES = [
    # W, H, n
    (50, 37, 1500),  # partial tiles on both edges, a tile with all eight neighbours
    (16, 16, 400),   # exactly one tile
    (17, 15, 400),   # one off the tile edge each way
    (15, 17, 400),
    (7, 5, 200),     # smaller than the tile and the window
    (1, 1, 50),      # the smallest image
]


@pytest.mark.parametrize("W,H,n", CASES, ids=[f"{c[0]}x{c[1]}" for c in CASES])
def test_kernel_matches_composed_image(mods, cuda, W, H, n):
    S = _state(mods, cuda, W, H, n)
    assert S["st"].num_pairs > 0 or W * H == 1  # (whether the one pixel is covered is the scene's business)
    _check(mods, cuda, S, f"{W}x{H}")


def test_more_than_256_tiles(mods, cuda):
    """260x257: 17 x 17 = 289 tiles, partial ones on both edges: the final kernel's stride-256 sum takes a second turn."""
    S = _state(mods, cuda, 260, 257, 2000)
    assert S["st"].num_pairs > 0
    _check(mods, cuda, S, "260x257")


@pytest.mark.parametrize("bg_dev", [False, True], ids=["background", "background_dev"])
def test_background(mods, cuda, bg_dev):
    S = _state(mods, cuda, 50, 37, 1500, BG, bg_dev)
    plain = _state(mods, cuda, 50, 37, 1500)
    assert not torch.equal(S["out"], plain["out"])  # (the background shows)
    got = _check(mods, cuda, S, "50x37 " + ("background_dev" if bg_dev else "background"))
    other = _metrics(mods, cuda, _state(mods, cuda, 50, 37, 1500, BG, not bg_dev)["st"], S["target"])
    assert torch.equal(got, other)  # both ways of passing it give the same colours


def test_view_without_pairs(mods, cuda):
    """Gaussians moved out of view: the metrics of the background image."""
    S = _state(mods, cuda, 50, 37, 300, BG, shift=1000.0)
    assert S["st"].num_pairs == 0
    assert torch.equal(S["out"], torch.tensor(BG, device=cuda).expand(37, 50, 3))
    _check(mods, cuda, S, "50x37 no pairs")


def test_target_equal_to_the_render(mods, cuda):
    S = _state(mods, cuda, 50, 37, 1500)
    got = _metrics(mods, cuda, S["st"], S["out"].clone())
    l1, mse, ssim = (float(x) for x in got)
    print(f"eval target = render: l1 {l1} mse {mse} ssim {ssim}")
    assert l1 <= ref.VALUE_TOL and mse <= ref.VALUE_TOL and abs(ssim - 1.0) <= ref.VALUE_TOL
    with_inf = -10.0 * math.log10(mse) if mse > 0.0 else math.inf
    assert math.isinf(with_inf)


def test_argument_checks_launch_nothing(mods, cuda):
    tr = mods[0]
    nat = tr._native
    L = nat.lib()
    S = _state(mods, cuda, 50, 37, 1500)
    st = S["st"]
    need = int(L.gr_eval_ws_bytes(ctypes.byref(st.gv)))
    assert need >= 3 * 4 * 12
    ws = torch.zeros((need,), dtype=torch.uint8, device=cuda)
    got = torch.full((3,), -1.0, device=cuda)
    stream = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)

    def call(gv, saved=st.saved, target=S["target"], out=got, wsp=ws, ws_bytes=need):
        return L.gr_eval_view(ctypes.byref(gv), nat.ptr(saved), nat.ptr(target), nat.ptr(out), nat.ptr(wsp), ws_bytes, stream)

    t32 = nat.GrView.from_buffer_copy(st.gv)
    t32.tile = 32
    assert call(t32) == nat.GR_ERR_INVALID_ARGUMENT
    band = nat.GrView.from_buffer_copy(st.gv)
    band.row0, band.rows = 0, 1
    assert call(band) == nat.GR_ERR_INVALID_ARGUMENT
    for kw in (dict(saved=None), dict(target=None), dict(out=None), dict(wsp=None)):
        assert call(st.gv, **kw) == nat.GR_ERR_INVALID_ARGUMENT
    assert call(st.gv, ws_bytes=need - 1) == nat.GR_ERR_WORKSPACE and b"workspace" in L.gr_last_error()
    with pytest.raises(ValueError):
        tr.eval_view_native(st, S["target"][:-1], got)
    torch.cuda.synchronize()
    assert bool((got == -1.0).all()) and not ws.any()  # a rejected call launches nothing
    assert call(st.gv) == nat.GR_OK
    torch.cuda.synchronize()
    assert bool((got != -1.0).all()) and ws.any()


def test_deterministic(mods, cuda):
    S = _state(mods, cuda, 50, 37, 1500)
    a = _metrics(mods, cuda, S["st"], S["target"])
    b = _metrics(mods, cuda, S["st"], S["target"])
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())


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
    """The six views' metrics by per-view forward_native + eval_view_native calls (computed once, left unchanged)."""
    tr, fm, _, bench = mods
    cams, targets, _ = scene
    p = bench.synthetic_params(FN, cuda)
    m, s, c, o = (t.detach().contiguous() for t in fm.activations(p))
    gvs = [tr.make_view(cam.view, cam.proj, FW, FH, None, depth_grad=False) for cam in cams]
    out = torch.zeros((FV, 3), device=cuda)
    for j, gv in enumerate(gvs):
        _, _, _, st = tr.forward_native(m, s, c, o, gv, images=False)
        tr.eval_view_native(st, targets[j], out[j])
    torch.cuda.synchronize()
    return (m, s, c, o), gvs, out


@pytest.mark.parametrize("streams", [1, 3])
def test_executor_matches_per_view_calls(mods, cuda, scene, per_view, streams):
    tr = mods[0]
    nat = tr._native
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
    got = [torch.full((FV, 3), -1.0, device=cuda) for _ in range(2)]
    for g in got:
        nat.check(nat.lib().gr_eval_views(nat.executor(cuda.index or 0), ctypes.byref(cfg), FV, arr, FN, nat.ptr(m), nat.ptr(s),
                                          nat.ptr(c), 3, nat.ptr(o), nat.ptr(g),
                                          ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)), "gr_eval_views")
    torch.cuda.synchronize()
    print(f"gr_eval_views, {streams} streams: {got[0].tolist()}")
    assert torch.equal(got[0], want) and torch.equal(got[1], want)
    assert bool((want[:, 0] > 0).all()) and bool((want[:, 1] > 0).all()) and bool(torch.isfinite(want).all())


def _with(fm, **kw):
    saved = {k: getattr(fm, k) for k in kw}
    for k, v in kw.items():
        setattr(fm, k, v)
    return saved


def test_fitter_evaluate(mods, cuda, scene):
    """evaluate() against the composed route.  On the fitter's own (Morton-ordered) activated parameters the image is
    the kernel's own input, so ssim is exact there; against render_gaussians_torch of the canonical parameters every
    metric is within VALUE_TOL (the order of the Gaussians may move the image's last bits; printed)."""
    tr, fm, losses, bench = mods
    cams, targets, masks = scene
    res = {}
    for native in ("1", "0"):
        saved = _with(fm, NATIVE_EXEC=native, NUM_STREAMS=3)
        try:
            f = fm.ViewShardedFitter(bench.synthetic_params(FN, cuda), cams, targets, FW, FH, masks=masks)
            f.step()
            res[native] = f.evaluate()
            assert f._eval_native_ok(cuda, targets) and f._native_exec() == (native == "1")
        finally:
            _with(fm, **saved)
    for k in res["1"]:
        assert (res["1"][k] == res["0"][k]).all() if hasattr(res["1"][k], "all") else res["1"][k] == res["0"][k], k
    got = res["0"]
    with torch.no_grad():
        own = [t.detach().contiguous() for t in fm.activations(f.params)]
        can = [t.detach().contiguous() for t in fm.activations(f.canonical_params())]
        exact = True
        for i, (cam, t) in enumerate(zip(cams, targets)):
            img, _, _, _ = tr.forward_native(*own, f._eval_view(cam, cuda))
            assert got["ssim"][i] == float(1.0 - losses.dssim_loss(img, t))
            d = img.double() - t.double()
            assert abs(got["l1"][i] - float(d.abs().mean())) <= ref.VALUE_TOL
            assert abs(got["mse"][i] - float((d * d).mean())) <= ref.VALUE_TOL
            user = tr.render_gaussians_torch(*can, cam, width=FW, height=FH, background=torch.zeros(3, device=cuda),
                                             depth_grad=False)
            want = losses.image_metrics(user, t)
            exact = exact and torch.equal(user, img)
            for k in ("l1", "mse", "ssim"):
                assert abs(got[k][i] - float(want[k])) <= ref.VALUE_TOL, (k, i)
            assert abs(got["psnr"][i] - (-10.0 * math.log10(got["mse"][i]))) <= 1e-12
    print(f"evaluate: PSNR {got['psnr'].tolist()} SSIM {got['ssim'].tolist()}; canonical-order image "
          f"{'bit-identical' if exact else 'differs in its last bits'}")
    # held-out views passed explicitly: the same numbers in the order passed
    sub = f.evaluate([cams[4], cams[1]], [targets[4], targets[1]])
    for k in ("l1", "mse", "psnr", "ssim"):
        assert sub[k].tolist() == [got[k][4], got[k][1]]


@pytest.mark.parametrize("mode", ["eager", "graph"])
@pytest.mark.parametrize("native", ["1", "0"], ids=["executor", "python"])
def test_evaluation_does_not_change_the_fit(mods, cuda, scene, mode, native):
    """Three steps against one step, evaluate(), two steps: losses, parameters, Adam moments and (eager: a fit that
    collects density statistics steps eagerly) density_state() bit for bit; graph: the captured batched step."""
    _, fm, _, bench = mods
    cams, targets, masks = scene
    saved = _with(fm, NATIVE_EXEC=native, GRAPH_MODE="0" if mode == "eager" else "batchgraph")
    try:
        runs = []
        for evaluate in (False, True):
            f = fm.ViewShardedFitter(bench.synthetic_params(FN, cuda), cams, targets, FW, FH, masks=masks,
                                     density_stats=mode == "eager")
            losses = [f.step()]
            assert f._graph_ok(cuda) == (mode == "graph")
            if evaluate:
                grads = {k: v.grad.detach().clone() for k, v in f.params.items()}
                r = f.evaluate()
                assert all(math.isfinite(r["mean_" + k]) for k in ("l1", "mse", "psnr", "ssim"))
                f.graph_sync()
                for k, v in f.params.items():
                    assert torch.equal(v.grad, grads[k]), k
            losses += [f.step() for _ in range(2)]
            f.graph_sync()
            torch.cuda.synchronize()
            runs.append(([float(x) for x in losses], {k: v.detach().clone() for k, v in f.params.items()},
                         {k: (f.opt.state[v]["exp_avg"].clone(), f.opt.state[v]["exp_avg_sq"].clone()) for k, v in f.params.items()},
                         f.density_state() if mode == "eager" else ()))
    finally:
        _with(fm, **saved)
    a, b = runs
    assert a[0] == b[0], (a[0], b[0])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
        assert torch.equal(a[2][k][0], b[2][k][0]) and torch.equal(a[2][k][1], b[2][k][1]), k
    for x, y in zip(a[3], b[3]):
        assert torch.equal(x, y) and float(x.sum()) > 0.0
