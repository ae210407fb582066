"""GPU: masked held-out metrics.  Kernel level: gr_eval_view_masked (k_eval_view_masked + k_eval_masked_final) on a
forward_native state, at tests/test_eval_gpu.py's shapes: a mask of ones against gr_eval_view bit for bit, a one-tile
mask against that tile's partial sums of gr_eval_view bit for bit, blob masks against the float64 restatement
(tests/eval_mask_reference.py) on the image and alpha the forward composes from the same state, an empty mask, a view
without pairs, both ways of passing a background, the call contract.  Executor level: gr_eval_views_masked against
per-view calls, bit for bit.  Fitter level: ViewShardedFitter.evaluate(masks=...) through the executor against the
Python schedule and against losses.image_metrics_masked of render_gaussians_torch, and a fit with such an evaluation in
it against the same fit without.

Tolerances.  Rows 0, 1, 2 and 4 are sums of non-negative terms: a float tree of at most 768 of them per tile is under
1e-6 relative, the tiles are summed in double, the values are at most 1: VALUE_TOL.  fg_ssim has the same bar for masks
covering at least 10 % of the image (asserted): a float32 SSIM map differs from the float64 one by up to 4.9e-6 in single
values, but by at most 2e-7 in masked means from 2 % coverage up (random targets, these shapes).  The IoU's counts are exact.

How fg_ssim is rounded: the device forms it as gr_eval_view forms its SSIM, 1 - float32(1 - sum / (3 M)), which is what
makes a mask of ones reproduce gr_eval_view bit for bit; the one-tile test therefore expects exactly that expression of the
tile's partial sum (and checks it is within one float32 step of 1.0, 6e-8, of the directly rounded quotient), while fg_l1
and fg_mse are float32(sum / (3 M)) as they stand."""
from __future__ import annotations

import ctypes
import importlib
import math

import numpy as np
import pytest
import torch

import eval_mask_reference as emr
import ssim_reference as ref

pytestmark = pytest.mark.gpu

BG = (0.2, 0.5, 0.7)
FW, FH, FV, FN = 96, 80, 6, 5000  # the fitter tests' shape (tests/test_eval_gpu.py)
NM, NK = 3, 6


@pytest.fixture(scope="module")
def mods(pkg, cuda):
    return (importlib.import_module("3dgaussian_amd.torch_renderer"), importlib.import_module("3dgaussian_amd.fit_multiview"),
            importlib.import_module("3dgaussian_amd.losses"), importlib.import_module("bench"))


_STATES: dict = {}


def _state(mods, cuda, W, H, n, bg=None, bg_dev=False, shift=0.0):
    """tests/test_eval_gpu.py's state: one view of n Gaussians on the orbit camera rendered once with images (shared, left
    unchanged) and a random target; here the alpha is kept too."""
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
        out, alpha, _, st = tr.forward_native(m, s, c, o, gv)
        torch.cuda.synchronize()
        _STATES[key] = dict(target=target, out=out, alpha=alpha, st=st, keep=bgt)
    return _STATES[key]


def _plain(mods, cuda, S):
    """gr_eval_view's three metrics and its workspace (the tiles' partial sums, planes of `plane` floats)."""
    nat = mods[0]._native
    L = nat.lib()
    st = S["st"]
    need = int(L.gr_eval_ws_bytes(ctypes.byref(st.gv)))
    ws = torch.zeros((need // 4,), dtype=torch.float32, device=cuda)
    got = torch.full((NM,), -1.0, device=cuda)
    nat.check(L.gr_eval_view(ctypes.byref(st.gv), nat.ptr(st.saved), nat.ptr(S["target"]), nat.ptr(got), nat.ptr(ws), need,
                             ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)), "gr_eval_view")
    torch.cuda.synchronize()
    return got, ws, need // 4 // NM


def _masked(mods, cuda, S, mask):
    """gr_eval_view_masked's row and its workspace (seven planes)."""
    nat = mods[0]._native
    L = nat.lib()
    st = S["st"]
    need = int(L.gr_eval_mask_ws_bytes(ctypes.byref(st.gv)))
    ws = torch.zeros((need // 4,), dtype=torch.float32, device=cuda)
    got = torch.full((NK,), -1.0, device=cuda)
    nat.check(L.gr_eval_view_masked(ctypes.byref(st.gv), nat.ptr(st.saved), nat.ptr(S["target"]), nat.ptr(mask), nat.ptr(got),
                                    nat.ptr(ws), need, ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)),
              "gr_eval_view_masked")
    torch.cuda.synchronize()
    return got, ws, need // 4 // 7


CASES = [
    # W, H, n
    (50, 37, 1500),  # partial tiles on both edges, a tile with all eight neighbours
    (16, 16, 400),   # exactly one tile
    (17, 15, 400),   # one off the tile edge each way
    (15, 17, 400),
    (7, 5, 200),     # smaller than the tile and the window
    (1, 1, 50),      # the smallest image
]
IDS = [f"{c[0]}x{c[1]}" for c in CASES]


@pytest.mark.parametrize("W,H,n", CASES, ids=IDS)
def test_mask_of_ones_is_gr_eval_view(mods, cuda, W, H, n):
    S = _state(mods, cuda, W, H, n)
    want, _, _ = _plain(mods, cuda, S)
    got, _, _ = _masked(mods, cuda, S, torch.ones((H, W), device=cuda))
    print(f"ones {W}x{H}: {got.tolist()} against gr_eval_view {want.tolist()}")
    assert torch.equal(got[1:4], want) and float(got[0]) == 1.0
    via = torch.full((NK,), -1.0, device=cuda)
    mods[0].eval_view_masked_native(S["st"], S["target"], torch.ones((H, W), device=cuda), via)
    assert torch.equal(via, got)


def test_one_interior_tile(mods, cuda):
    W, H = 50, 37
    S = _state(mods, cuda, W, H, 1500)
    _, ws, plane = _plain(mods, cuda, S)
    tile = 1 * 4 + 1  # tile (1, 1) of 4 x 3: all eight neighbours
    mask = torch.zeros((H, W), device=cuda)
    mask[16:32, 16:32] = 1.0
    got, _, _ = _masked(mods, cuda, S, mask)
    part = [np.float64(float(ws[q * plane + tile])) for q in range(3)]  # q = 0 the SSIM sum, 1 |d|, 2 d^2
    n = 3.0 * 256.0
    want_l1, want_mse = np.float32(part[1] / n), np.float32(part[2] / n)
    want_ssim = np.float32(1.0) - np.float32(1.0 - part[0] / n)  # as gr_eval_view forms its SSIM (the module docstring)
    print(f"one tile: {got.tolist()} against partials {part}")
    assert float(got[0]) == float(np.float32(256.0 / (H * W)))
    assert float(got[1]) == float(want_l1) and float(got[2]) == float(want_mse)
    assert float(got[3]) == float(want_ssim)
    assert abs(float(got[3]) - float(np.float32(part[0] / n))) <= 2.0 ** -24


def _check_ref(mods, cuda, S, mask, tag, coverage=True):
    """Rows 0..4 within VALUE_TOL of the float64 restatement on the composed image and alpha; the IoU's counts exact."""
    got, ws, plane = _masked(mods, cuda, S, mask)
    want = emr.metrics(S["out"], S["alpha"], S["target"], mask)
    print(f"masked {tag}: " + " ".join(f"{k} {float(got[q]):.8f} (f64 {want[k]:.8f})" for q, k in enumerate(emr.KEYS))
          + f" I {want['inter']} U {want['union']}")
    if coverage:
        assert want["fg_fraction"] >= 0.1  # the condition of fg_ssim's bar
        for q in range(5):
            assert abs(float(got[q]) - want[emr.KEYS[q]]) <= ref.VALUE_TOL, emr.KEYS[q]
    inter, union = float(ws[5 * plane:6 * plane].double().sum()), float(ws[6 * plane:7 * plane].double().sum())
    assert (inter, union) == (want["inter"], want["union"])
    assert float(got[5]) == float(np.float32(want["sil_iou"]))
    return got, want


@pytest.mark.parametrize("soft", [False, True], ids=["binary", "soft"])
@pytest.mark.parametrize("W,H,n", CASES, ids=IDS)
def test_blob_masks_match_float64(mods, cuda, W, H, n, soft):
    S = _state(mods, cuda, W, H, n)
    mask = emr.blob_mask(H, W, soft).to(cuda)
    assert bool((mask == 0.5).any())  # exactly the threshold: counts as "not above"
    _check_ref(mods, cuda, S, mask, f"{W}x{H} {'soft' if soft else 'binary'}")


def test_more_than_256_tiles(mods, cuda):
    """260x257: 17 x 17 = 289 tiles, partial ones on both edges: the final kernel's stride-256 sums take a second turn."""
    S = _state(mods, cuda, 260, 257, 2000)
    assert S["st"].num_pairs > 0
    _check_ref(mods, cuda, S, emr.blob_mask(257, 260, False).to(cuda), "260x257 binary")


@pytest.mark.parametrize("W,H,n", CASES, ids=IDS)
def test_mask_of_zeros(mods, cuda, W, H, n):
    S = _state(mods, cuda, W, H, n)
    got, want = _check_ref(mods, cuda, S, torch.zeros((H, W), device=cuda), f"{W}x{H} zeros", coverage=False)
    assert got[:4].tolist() == [0.0, 0.0, 0.0, 0.0] and want["inter"] == 0
    assert abs(float(got[4]) - float(S["alpha"].double().mean())) <= ref.VALUE_TOL
    assert float(got[5]) == (0.0 if want["union"] else 1.0)


def test_view_without_pairs(mods, cuda):
    """Gaussians moved out of view: alpha = 0 everywhere, the colours are the background's."""
    S = _state(mods, cuda, 50, 37, 300, BG, shift=1000.0)
    assert S["st"].num_pairs == 0 and not S["alpha"].any()
    assert torch.equal(S["out"], torch.tensor(BG, device=cuda).expand(37, 50, 3))
    mask = emr.blob_mask(37, 50, True).to(cuda)
    got, want = _check_ref(mods, cuda, S, mask, "50x37 no pairs")
    assert abs(float(got[4]) - float(mask.double().mean())) <= ref.VALUE_TOL
    assert bool((mask > 0.5).any()) and float(got[5]) == 0.0 and want["inter"] == 0 and want["union"] > 0


@pytest.mark.parametrize("bg_dev", [False, True], ids=["background", "background_dev"])
def test_background(mods, cuda, bg_dev):
    S = _state(mods, cuda, 50, 37, 1500, BG, bg_dev)
    assert not torch.equal(S["out"], _state(mods, cuda, 50, 37, 1500)["out"])  # (the background shows)
    mask = emr.blob_mask(37, 50, True).to(cuda)
    got, _ = _check_ref(mods, cuda, S, mask, "50x37 " + ("background_dev" if bg_dev else "background"))
    other, _, _ = _masked(mods, cuda, _state(mods, cuda, 50, 37, 1500, BG, not bg_dev), mask)
    assert torch.equal(got, other)  # both ways of passing it give the same rows


def test_argument_checks_launch_nothing(mods, cuda):
    tr = mods[0]
    nat = tr._native
    L = nat.lib()
    S = _state(mods, cuda, 50, 37, 1500)
    st = S["st"]
    need = int(L.gr_eval_mask_ws_bytes(ctypes.byref(st.gv)))
    assert need >= 7 * 4 * 12
    ws = torch.zeros((need,), dtype=torch.uint8, device=cuda)
    got = torch.full((NK,), -1.0, device=cuda)
    mask = emr.blob_mask(37, 50, True).to(cuda)
    stream = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)

    def call(gv, saved=st.saved, target=S["target"], msk=mask, out=got, wsp=ws, ws_bytes=need):
        return L.gr_eval_view_masked(ctypes.byref(gv), nat.ptr(saved), nat.ptr(target), nat.ptr(msk), nat.ptr(out),
                                     nat.ptr(wsp), ws_bytes, stream)

    t32 = nat.GrView.from_buffer_copy(st.gv)
    t32.tile = 32
    assert call(t32) == nat.GR_ERR_INVALID_ARGUMENT
    band = nat.GrView.from_buffer_copy(st.gv)
    band.row0, band.rows = 0, 1
    assert call(band) == nat.GR_ERR_INVALID_ARGUMENT
    for kw in (dict(saved=None), dict(target=None), dict(msk=None), dict(out=None), dict(wsp=None)):
        assert call(st.gv, **kw) == nat.GR_ERR_INVALID_ARGUMENT, kw
    assert call(st.gv, ws_bytes=need - 1) == nat.GR_ERR_WORKSPACE and b"workspace" in L.gr_last_error()
    for bad in (mask[:-1], mask.double(), mask.cpu(), mask.t(), None):  # shape, dtype, device, layout, missing
        with pytest.raises(ValueError):
            tr.eval_view_masked_native(st, S["target"], bad, got)
    with pytest.raises(ValueError):
        tr.eval_view_masked_native(st, S["target"][:-1], mask, got)
    torch.cuda.synchronize()
    assert bool((got == -1.0).all()) and not ws.any()  # a rejected call launches nothing
    assert call(st.gv) == nat.GR_OK
    torch.cuda.synchronize()
    assert bool((got != -1.0).all()) and ws.any()


def test_deterministic(mods, cuda):
    S = _state(mods, cuda, 50, 37, 1500)
    mask = emr.blob_mask(37, 50, True).to(cuda)
    a, wa, _ = _masked(mods, cuda, S, mask)
    b, wb, _ = _masked(mods, cuda, S, mask)
    assert torch.equal(a, b) and torch.equal(wa, wb) and bool(torch.isfinite(a).all())


# ---- executor and fitter level ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(mods, cuda):
    fm = mods[1]
    cams = fm.orbit_cameras(FV, FW, FH, cuda)
    g = torch.Generator(device=cuda).manual_seed(9)
    targets = [torch.rand((FH, FW, 3), generator=g, device=cuda) for _ in cams]
    masks = [(t.mean(dim=2) > 0.5).float() for t in targets]
    held = [emr.blob_mask(FH, FW, soft=bool(i % 2), seed=i).to(cuda) for i in range(FV)]  # masks that are not the fit's
    return cams, targets, masks, held


@pytest.fixture(scope="module")
def per_view(mods, cuda, scene):
    """The six views' rows by per-view forward_native + eval_view_native + eval_view_masked_native calls (computed once,
    left unchanged)."""
    tr, fm, _, bench = mods
    cams, targets, _, held = scene
    p = bench.synthetic_params(FN, cuda)
    m, s, c, o = (t.detach().contiguous() for t in fm.activations(p))
    gvs = [tr.make_view(cam.view, cam.proj, FW, FH, None, depth_grad=False) for cam in cams]
    out = torch.zeros((FV, NM + NK), device=cuda)
    for j, gv in enumerate(gvs):
        _, _, _, st = tr.forward_native(m, s, c, o, gv, images=False)
        tr.eval_view_native(st, targets[j], out[j, :NM])
        tr.eval_view_masked_native(st, targets[j], held[j], out[j, NM:])
    torch.cuda.synchronize()
    return (m, s, c, o), gvs, out


@pytest.mark.parametrize("streams", [1, 3])
def test_executor_matches_per_view_calls(mods, cuda, scene, per_view, streams):
    tr = mods[0]
    nat = tr._native
    (m, s, c, o), gvs, want = per_view
    _, targets, _, held = scene
    arr = (nat.GrFitTarget * FV)()
    for j in range(FV):
        arr[j].view = gvs[j]
        arr[j].target_rgb = targets[j].data_ptr()
        arr[j].target_mask = held[j].data_ptr()
    side = [torch.cuda.Stream(cuda) for _ in range(streams - 1)]
    prep = torch.cuda.Stream(cuda)
    cfg = nat.GrFitConfig(streams, 6, 4, 1, 0, 0)  # (reduce_batch / reduce_tail are ignored)
    rs = (ctypes.c_void_p * max(1, streams - 1))(*[x.cuda_stream for x in side])
    cfg.render_streams = rs
    cfg.prep_stream = prep.cuda_stream
    ex = nat.executor(cuda.index or 0)
    cur = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    args = (ctypes.byref(cfg), FV, arr, FN, nat.ptr(m), nat.ptr(s), nat.ptr(c), 3, nat.ptr(o))
    got = [torch.full((FV, NM + NK), -1.0, device=cuda) for _ in range(2)]
    for g in got:
        nat.check(nat.lib().gr_eval_views_masked(ex, *args, nat.ptr(g), cur), "gr_eval_views_masked")
    plain = torch.full((FV, NM), -1.0, device=cuda)
    nat.check(nat.lib().gr_eval_views(ex, *args, nat.ptr(plain), cur), "gr_eval_views")
    torch.cuda.synchronize()
    print(f"gr_eval_views_masked, {streams} streams: {got[0].tolist()}")
    assert torch.equal(got[0], want) and torch.equal(got[1], want)
    assert torch.equal(got[0][:, :NM], plain)
    assert bool(torch.isfinite(want).all()) and bool((want[:, NM] >= 0.1).all())
    # a view without a mask is refused before anything is enqueued
    arr[2].target_mask = None
    none = torch.full((FV, NM + NK), -1.0, device=cuda)
    assert nat.lib().gr_eval_views_masked(ex, *args, nat.ptr(none), cur) == nat.GR_ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert bool((none == -1.0).all())


def _with(fm, **kw):
    saved = {k: getattr(fm, k) for k in kw}
    for k, v in kw.items():
        setattr(fm, k, v)
    return saved


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


def test_fitter_evaluate(mods, cuda, scene):
    """evaluate(masks=...): the executor against the Python schedule key by key; against losses.image_metrics_masked on
    render_gaussians_torch's image and alpha of the canonical parameters within VALUE_TOL (the IoU as a value: the order of
    the Gaussians may move the image's last bits); the plain keys, masks=True and a sub-list of views."""
    tr, fm, losses, bench = mods
    cams, targets, masks, held = scene
    res, plain, own = {}, {}, {}
    for native in ("1", "0"):
        saved = _with(fm, NATIVE_EXEC=native, NUM_STREAMS=3)
        try:
            f = fm.ViewShardedFitter(bench.synthetic_params(FN, cuda), cams, targets, FW, FH, masks=masks)
            f.step()
            res[native] = f.evaluate(masks=held)
            plain[native] = f.evaluate()
            own[native] = (f.evaluate(masks=True), f.evaluate(masks=masks))
            sub = f.evaluate([cams[4], cams[1]], [targets[4], targets[1]], masks=[held[4], held[1]])
            assert f._eval_native_ok(cuda, targets) and f._native_exec() == (native == "1")
        finally:
            _with(fm, **saved)
        _same(*own[native])  # masks=True: the training masks
        for k in plain[native]:  # the plain keys keep their bits
            assert np.array_equal(np.asarray(res[native][k]), np.asarray(plain[native][k])), k
        for k in res[native]:
            if not k.startswith("mean_"):
                assert sub[k].tolist() == [res[native][k][4], res[native][k][1]], k
    _same(res["1"], res["0"])
    _same(own["1"][0], own["0"][0])
    got = res["0"]
    with torch.no_grad():
        can = [t.detach().contiguous() for t in fm.activations(f.canonical_params())]
        for i, (cam, t) in enumerate(zip(cams, targets)):
            user, alpha, _ = tr.render_gaussians_torch(*can, cam, width=FW, height=FH, background=torch.zeros(3, device=cuda),
                                                       depth_grad=False, return_aux=True)
            want = losses.image_metrics_masked(user, alpha, t, held[i])
            assert float(want["fg_fraction"]) >= 0.1
            for k in ("fg_fraction", "fg_l1", "fg_mse", "fg_ssim", "sil_l1"):
                assert abs(got[k][i] - float(want[k])) <= ref.VALUE_TOL, (k, i)
            assert abs(got["sil_iou"][i] - float(want["sil_iou"].float())) <= 1e-12, i  # (the row holds float32 values)
            assert abs(got["fg_psnr"][i] - (-10.0 * math.log10(got["fg_mse"][i]))) <= 1e-12
    for k in emr.KEYS + ("fg_psnr",):
        assert got["mean_" + k] == float(got[k].mean()), k
    print(f"evaluate(masks): fg PSNR {got['fg_psnr'].tolist()} (whole {got['psnr'].tolist()}) IoU {got['sil_iou'].tolist()}")


@pytest.mark.parametrize("mode", ["eager", "graph"])
@pytest.mark.parametrize("native", ["1", "0"], ids=["executor", "python"])
def test_evaluation_does_not_change_the_fit(mods, cuda, scene, mode, native):
    """Three steps against one step, evaluate(masks=True), two steps: losses, parameters and Adam moments bit for bit;
    graph: the captured batched step."""
    _, fm, _, bench = mods
    cams, targets, masks, _ = scene
    saved = _with(fm, NATIVE_EXEC=native, GRAPH_MODE="0" if mode == "eager" else "batchgraph")
    try:
        runs = []
        for evaluate in (False, True):
            f = fm.ViewShardedFitter(bench.synthetic_params(FN, cuda), cams, targets, FW, FH, masks=masks)
            losses = [f.step()]
            assert f._graph_ok(cuda) == (mode == "graph")
            if evaluate:
                grads = {k: v.grad.detach().clone() for k, v in f.params.items()}
                r = f.evaluate(masks=True)
                assert all(math.isfinite(r["mean_" + k]) for k in emr.KEYS + ("fg_psnr", "psnr"))
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
