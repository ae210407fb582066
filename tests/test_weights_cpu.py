"""CPU: per-pixel loss weights in the fit (ViewShardedFitter(weights=...), the CLI's --weights_dir) on host tensors
against the float64 restatement tests/weights_reference.py; ones are the fit without weights bit for bit; a zero weight
hides a pixel's targets; a painted distractor; validation; the refusals of gr_bwd_fit_weighted_gather that return before
any device call; the CLI's files."""
from __future__ import annotations

import ctypes
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import exposure_reference as eref  # noqa: E402
import weights_reference as wref  # noqa: E402

GRAD_TOL = 1e-4  # tests/test_exposure_cpu.py's gradient bar for its forms: relative L2
LOSS_TOL = 2e-6  # ... and its loss bar
W, H, V = eref.W, eref.H, eref.V
RECT = (10, 6, 24, 18)  # the zero rectangle (x0, y0, x1, y1): all of no 16-pixel tile at 32 x 24, part of all four


@pytest.fixture(scope="module")
def fm():
    return importlib.import_module("3dgaussian_amd.fit_multiview")


def _cams(device=torch.device("cpu")):
    tr = importlib.import_module("3dgaussian_amd.torch_renderer")
    cams = orc.orbit_cameras(V, W, H)
    return cams, [tr.Camera(view=torch.from_numpy(np.asarray(v, np.float32)).to(device),
                            proj=torch.from_numpy(np.asarray(p, np.float32)).to(device)) for v, p in cams]


def _weights(seed=0):
    return [wref.weight_map(W, H, RECT, seed + i) for i in range(V)]


def _inside(t, value):
    """t with the zero rectangle's values replaced."""
    t = t.clone()
    x0, y0, x1, y1 = RECT
    t[y0:y1, x0:x1] = value
    return t


def _small_setup(fm, n=60, depths=False):
    torch.manual_seed(7)
    dev = torch.device("cpu")
    params = fm.build_params(n, dev, use_sh=False)
    with torch.no_grad():
        params["scales_raw"].fill_(-1.5)
    cams = fm.orbit_cameras(V, W, H, dev)
    g = torch.Generator().manual_seed(3)
    targets = [torch.rand((H, W, 3), generator=g) for _ in range(V)]
    masks = [(t.mean(2) > 0.5).float() for t in targets]
    dep = [torch.rand((H, W), generator=g) for _ in range(V)] if depths else None
    return params, cams, targets, masks, dep


def _run(fit, steps=3):
    losses = [fit.step().clone() for _ in range(steps)]
    return losses, {k: v.detach().clone() for k, v in fit.params.items()}


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and all(torch.equal(a[1][k], b[1][k]) for k in a[1])


def test_the_gpu_tests_weight_maps():
    """The zero rectangles of tests/test_weights_gpu.py cover what that file says: at 50 x 37 all of one tile and part of
    its eight neighbours, about a quarter of the pixels; every partly covered tile keeps a pixel with a positive weight."""
    for (w, h), rect in wref.GPU_RECTS.items():
        m = wref.weight_map(w, h, rect, wref.GPU_WEIGHT_SEED)
        assert m.dtype == torch.float32 and float(m[m > 0].min()) >= 0.25 and float(m.max()) <= 4.0
        cover = wref.tile_cover(m)
        part = sorted(k for k, (n_all, n_pos) in cover.items() if 0 < n_pos < n_all)
        full = [k for k, (n_all, n_pos) in cover.items() if n_pos == 0]
        assert part and full == ([(1, 1)] if (w, h) == (50, 37) else [])
        if (w, h) == (50, 37):
            assert len(cover) == 12 and part == [(a, b) for a in range(3) for b in range(3) if (a, b) != (1, 1)]
            zeros = sum(n_all - n_pos for n_all, n_pos in cover.values())
            assert zeros == 480 and 0.2 <= zeros / (w * h) <= 0.3


# ---- 1. the host fitter against the float64 reference ----------------------------------------------------------------
@pytest.mark.parametrize("form", ["l1", "depth"])
def test_host_fitter_matches_the_reference(fm, form):
    """Per-view loss and the gradients of all four parameters against weights_reference on the dense float64 render
    (targets and depth targets kept 1e-3 from the kinks: the float32 render's signs are the reference's)."""
    scene = eref.scene_arrays(1)
    cams, fc = _cams()
    g = torch.Generator().manual_seed(4)
    weights = _weights()
    assert all(0 < n_pos < n_all for n_all, n_pos in wref.tile_cover(weights[0]).values())
    targets, depths = [], []
    for view, proj in cams:
        out, _, depth = eref.exposed(wref.dense_sums(*scene, view, proj, W, H), None, torch.eye(3, 4))[1:]
        targets.append(wref.clear_targets(out, torch.rand((H, W, 3), generator=g)))
        depths.append(wref.clear_targets(depth / (depth.max() + 1e-6), torch.rand((H, W), generator=g)))
    masks = [(t.mean(2) > 0.5).float() for t in targets] if form == "depth" else None
    depths = depths if form == "depth" else None
    fit = fm.ViewShardedFitter(eref.exact_params(scene, torch.device("cpu")), fc, targets, W, H, lr=0.0, masks=masks,
                               depths=depths, weights=weights, reorder=False)
    raw = {k: v.detach().clone() for k, v in fit.params.items()}
    with torch.no_grad():
        acts = fm.activations(fit.params)
        per = [float(fit.view_loss(i, *acts)) for i in range(V)]
    loss = float(fit.step())
    w_sil = fit.w_sil if masks is not None else 0.0
    ref_per, ref_total, ref_g = wref.fit_loss_and_grads(raw, cams, W, H, weights, targets, masks, w_sil, depths, fit.w_depth,
                                                        fit.reg_opacity, fit.reg_scale)
    print(f"{form}: view losses {per} reference {ref_per}; step loss {loss:.7f} reference {ref_total:.7f}")
    assert all(abs(a - b) <= LOSS_TOL for a, b in zip(per, ref_per)) and abs(loss - ref_total) <= LOSS_TOL
    for k, p in fit.params.items():
        want = ref_g[k]
        rel = float((p.grad.double() - want).norm() / want.norm())
        print(f"  d loss / d {k}: relL2 {rel:.2e} (bar {GRAD_TOL:.0e})")
        assert float(want.norm()) > 0 and rel <= GRAD_TOL, k


# ---- 2. ones are the fit without weights ----------------------------------------------------------------------------
@pytest.mark.parametrize("depths", [False, True])
def test_ones_are_off(fm, depths):
    runs = []
    for on in (False, True):
        params, cams, targets, masks, dep = _small_setup(fm, depths=depths)
        kw = {"weights": [torch.ones((H, W)) for _ in range(V)]} if on else {}
        fit = fm.ViewShardedFitter(params, cams, targets, W, H, masks=masks, depths=dep, **kw)
        runs.append(_run(fit))
        assert (fit.weights is not None) == on
    assert _same(*runs)


def test_ones_are_off_beside_exposure(fm):
    runs = []
    for on in (False, True):
        params, cams, targets, masks, _ = _small_setup(fm)
        kw = {"weights": [torch.ones((H, W), dtype=torch.float64) for _ in range(V)]} if on else {}
        fit = fm.ViewShardedFitter(params, cams, targets, W, H, masks=masks, exposure=True, **kw)
        runs.append(_run(fit) + (fit.exposure_state()[0],))
    assert _same(runs[0], runs[1]) and torch.equal(runs[0][2], runs[1][2])


# ---- 3. a zero weight hides the pixel's targets -------------------------------------------------------------------------
def test_zero_weight_independence(fm):
    runs = []
    for change in (False, True):
        params, cams, targets, masks, dep = _small_setup(fm, depths=True)
        if change:
            targets = [_inside(t, 1.0 - t[RECT[1]:RECT[3], RECT[0]:RECT[2]]) for t in targets]
            masks = [_inside(m, 1.0 - m[RECT[1]:RECT[3], RECT[0]:RECT[2]]) for m in masks]
            dep = [_inside(d, 0.5) for d in dep]
        fit = fm.ViewShardedFitter(params, cams, targets, W, H, masks=masks, depths=dep, weights=_weights())
        runs.append(_run(fit))
    assert _same(*runs)
    # (and the weights are not ignored: the same fit without them differs)
    params, cams, targets, masks, dep = _small_setup(fm, depths=True)
    plain = _run(fm.ViewShardedFitter(params, cams, targets, W, H, masks=masks, depths=dep))
    assert not _same(runs[0], plain)


# ---- 4. a distractor -----------------------------------------------------------------------------------------------------
def test_distractor(fm):
    """Exact Gaussians, targets rendered from them, a bright square painted into two views' targets: with zero weights
    over the square the fit does not see it (equal to the weighted fit on clean targets), and stays closer to the truth
    than the unweighted fit on the painted targets."""
    scene = eref.scene_arrays(5)
    cams, fc = _cams()
    clean = [eref.exposed(wref.dense_sums(*scene, view, proj, W, H), None, torch.eye(3, 4))[1].to(torch.float32)
             for view, proj in cams]
    painted = [_inside(t, 1.0) if i in (1, 2) else t.clone() for i, t in enumerate(clean)]
    weights = [_inside(torch.ones((H, W)), 0.0) if i in (1, 2) else torch.ones((H, W)) for i in range(V)]
    truth = eref.exact_params(scene, torch.device("cpu"))

    def fit(targets, w):
        f = fm.ViewShardedFitter(eref.exact_params(scene, torch.device("cpu")), fc, targets, W, H, lr=0.002, masks=None,
                                 reg_opacity=0.0, reg_scale=0.0, weights=w, reorder=False)
        for _ in range(40):
            f.step()
        return {k: v.detach().clone() for k, v in f.params.items()}

    def drift(p):
        return float(sum((p[k] - truth[k].detach()).abs().sum() for k in p) / sum(p[k].numel() for k in p))

    a, b, c = fit(painted, weights), fit(clean, weights), fit(painted, None)
    print(f"mean parameter drift after 40 steps: weighted on painted targets {drift(a):.5f}, unweighted {drift(c):.5f}")
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert drift(a) < drift(c)


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------
def test_validation(fm, tmp_path):
    params, cams, targets, masks, _ = _small_setup(fm)
    ones = [torch.ones((H, W)) for _ in range(V)]

    def make(weights, **kw):
        return fm.ViewShardedFitter(params, cams, targets, W, H, masks=masks, weights=weights, **kw)

    with pytest.raises(ValueError, match=r"weights: expected one map per training view \(4\), got 3"):
        make(ones[:3])
    with pytest.raises(ValueError, match=r"weights\[1\]: expected shape \(24, 32\)"):
        make([ones[0], torch.ones((W, H)), ones[2], ones[3]])
    with pytest.raises(ValueError, match=r"weights\[0\]: expected shape \(24, 32\)"):
        make([torch.ones((H, W, 1))] + ones[1:])
    for bad in (torch.ones((H, W), dtype=torch.int64), torch.ones((H, W), dtype=torch.bool),
                torch.ones((H, W), dtype=torch.uint8)):
        with pytest.raises(ValueError, match=r"weights\[2\]: expected a floating-point dtype"):
            make(ones[:2] + [bad] + ones[3:])
    neg = ones[3].clone()
    neg[5, 7] = -0.5
    with pytest.raises(ValueError, match=r"weights\[3\]: every weight must be >= 0, got a minimum of -0.5"):
        make(ones[:3] + [neg])
    for v in (float("nan"), float("inf")):
        bad = ones[0].clone()
        bad[0, 0] = v
        with pytest.raises(ValueError, match=r"weights\[0\]: every weight must be finite"):
            make([bad] + ones[1:])
    with pytest.raises(ValueError, match=r"weights\[0\]: every weight must be finite"):  # (finite in float64 only)
        make([torch.full((H, W), 1e300, dtype=torch.float64)] + ones[1:])
    with pytest.raises(ValueError, match="weights with dssim_weight > 0"):
        make(ones, dssim_weight=0.2)
    with pytest.raises(ValueError, match="weights with dssim_weight > 0"):
        make(ones, dssim_weight=0.2, dssim_fused=True)
    fit = make([w.double().numpy() for w in ones])  # float64 arrays are converted
    assert all(w.dtype == torch.float32 and w.is_contiguous() for w in fit.weights) and fit._images_ok
    assert fit._form() != "weighted" and not fit._wgt_dev  # host tensors: view_loss, no device form
    # the CLI: a training view without a file
    wdir = tmp_path / "w"
    wdir.mkdir()
    np.save(wdir / "v0.npy", np.ones((24, 32), np.float32))
    np.save(wdir / "v2.npy", np.ones((24, 32), np.float32))
    with pytest.raises(FileNotFoundError, match=r"--weights_dir: no weight map for training view 'v1' \(v1.npy or v1.png\)"):
        fm.main(_main_args(tmp_path / "bad", "--weights_dir", str(wdir)))
    np.save(wdir / "v1.npy", np.ones((24, 31), np.float32))
    with pytest.raises(ValueError, match=r"weights\[1\]: expected shape \(24, 32\)"):
        fm.main(_main_args(tmp_path / "bad", "--weights_dir", str(wdir)))
    with pytest.raises(ValueError, match="weights with dssim_weight > 0"):
        np.save(wdir / "v1.npy", np.ones((24, 32), np.float32))
        fm.main(_main_args(tmp_path / "bad", "--weights_dir", str(wdir), "--dssim_weight", "0.2"))


# ---- 6. the ABI's refusals before any device call (in the manner of test_bwd_request_cpu.py) ------------------------------
INVALID, WORKSPACE = 1, 3  # GR_ERR_INVALID_ARGUMENT, GR_ERR_WORKSPACE
N = 10
ENTRY = "gr_bwd_fit_weighted_gather"
_BUF = (ctypes.c_float * 4)()
P = ctypes.cast(_BUF, ctypes.c_void_p)  # a non-null pointer (never dereferenced)
NULL = ctypes.c_void_p(0)
F = ctypes.c_float
TILE32 = "32-pixel tiles (gr_view.tile = 32): the fused fit path only (gr_bwd_splat)"
ROWS = "a band of tile rows (gr_view.rows): the fused fit path only (gr_bwd_splat)"
DEPTH = "depth gradient for a view rendered with no_depth_grad (render it with depth_grad=True)"


def _abi_cases(pkg):
    nat = pkg._native
    mk = lambda dg: pkg.torch_renderer.make_view(np.eye(4, dtype="float32"), np.eye(4, dtype="float32"), 40, 24,  # noqa: E731
                                                 depth_grad=dg)
    base, flat = mk(True), mk(False)
    assert base.no_depth_grad == 0 and flat.no_depth_grad == 1

    def view(src=base, **fields):
        v = nat.GrView.from_buffer_copy(src)
        for k, val in fields.items():
            setattr(v, k, val)
        return v

    own = lambda what: f"{ENTRY}: {what} is null"  # noqa: E731
    return base, [
        # what, operand overrides, status, message
        ("null target_weight", dict(weight=NULL), INVALID, own("target_weight")),
        ("null target_rgb", dict(target=NULL), INVALID, own("target_rgb")),
        ("null sums", dict(sums=NULL), INVALID, own("sums")),
        # the entry's own operands in its order (target_rgb, sums, target_weight), all before the view's checks
        ("null target_rgb, sums, target_weight", dict(target=NULL, sums=NULL, weight=NULL), INVALID, own("target_rgb")),
        ("null sums, target_weight", dict(sums=NULL, weight=NULL), INVALID, own("sums")),
        ("null target_weight, null view", dict(weight=NULL, view=None), INVALID, own("target_weight")),
        ("null target_weight, tile 32", dict(weight=NULL, view=view(tile=32)), INVALID, own("target_weight")),
        ("null target_weight, short workspace", dict(weight=NULL, ws_bytes=0), INVALID, own("target_weight")),
        ("null view", dict(view=None), INVALID, "view is null"),
        ("null plan", dict(plan=None), INVALID, "plan is null"),
        ("tile 32", dict(view=view(tile=32)), INVALID, TILE32),
        ("rows > 0", dict(view=view(rows=1)), INVALID, ROWS),
        ("tile 32, rows > 0, null plan", dict(view=view(tile=32, rows=1), plan=None), INVALID, TILE32),
        ("rows > 0, null plan", dict(view=view(rows=1), plan=None), INVALID, ROWS),
        ("depth target, no_depth_grad view", dict(view=flat, tdepth=P), INVALID, DEPTH),
        ("depth target, no_depth_grad view, tile 32", dict(view=view(flat, tile=32), tdepth=P), INVALID, DEPTH),
        ("null loss", dict(loss=NULL), INVALID, "gr_bwd_l1: null loss or workspace"),
        ("null loss, short workspace", dict(loss=NULL, ws_bytes=0), INVALID, "gr_bwd_l1: null loss or workspace"),
        # the workspace is gr_bwd_bytes: one byte less is refused, exactly that passes every check up to the launch (not
        # tried here); tile and rows come before the workspace
        ("workspace one byte short", dict(ws_bytes=-1), WORKSPACE, "backward workspace too small"),
        ("tile 32, workspace one byte short", dict(view=view(tile=32), ws_bytes=-1), INVALID, TILE32),
        ("rows > 0, workspace one byte short", dict(view=view(rows=1), ws_bytes=-1), INVALID, ROWS),
    ]


def test_abi_refusals(pkg):
    nat = pkg._native
    L = nat.lib()
    base, cases = _abi_cases(pkg)
    for what, over, status, message in cases:
        a = dict(view=base, plan=nat.GrPlan(100, 200, 100), target=P, mask=NULL, tdepth=NULL, weight=P, loss=P, sums=P,
                 ws_bytes=1 << 40)
        a.update(over)
        if a["ws_bytes"] == -1:
            a["ws_bytes"] = L.gr_bwd_bytes(ctypes.byref(a["view"]), N, ctypes.byref(a["plan"])) - 1
        got = L.gr_bwd_fit_weighted_gather(
            ctypes.byref(a["view"]) if a["view"] is not None else None, N,
            ctypes.byref(a["plan"]) if a["plan"] is not None else None, P, P, P, a["target"], a["mask"], F(0.2), a["tdepth"],
            F(0.05), F(0.25), a["weight"], a["loss"], P, a["ws_bytes"], a["sums"], P, NULL)
        assert (got, L.gr_last_error().decode()) == (status, message), what
    # n == 0 is a no-op once the view and the plan passed
    got = L.gr_bwd_fit_weighted_gather(ctypes.byref(base), 0, ctypes.byref(nat.GrPlan(0, 0, 0)), P, P, P, P, NULL, F(0.2),
                                       NULL, F(0.0), F(0.25), P, P, P, 0, P, P, NULL)
    assert got == 0


def test_wrapper_checks_the_weight_before_any_call(pkg):
    tr = pkg.torch_renderer
    gv = tr.make_view(np.eye(4, dtype="float32"), np.eye(4, dtype="float32"), 40, 24, depth_grad=False)
    dev = torch.device("cpu")
    ok = torch.ones((24, 40))
    tr._check_targets(gv, torch.ones((24, 40, 3)), None, None, dev, ok)
    for bad in (torch.ones((40, 24)), ok.double(), torch.ones((24, 80))[:, ::2], torch.ones((24, 40), device="meta")):
        with pytest.raises(ValueError, match="weight: expected a contiguous float32 tensor of shape"):
            tr._check_targets(gv, torch.ones((24, 40, 3)), None, None, dev, bad)
    with pytest.raises(ValueError, match="weight: expected a contiguous float32 tensor"):
        tr.backward_fit_weighted_gather_native(None, None, None, 0.0, None, 0.0, 1.0, None, None)
    row = pkg._native._SIG[ENTRY][1]
    assert len(row) == len(pkg._native._SIG["gr_bwd_fit_gather"][1]) + 1  # gr_bwd_fit_gather's list plus the weight


# ---- 7. the CLI ------------------------------------------------------------------------------------------------------------
def _main_args(out, *extra):
    return ["--targets_dir", os.path.join(GOLDEN, "fit_targets"), "--out_dir", str(out), "--iters", "3", "--width", "32",
            "--height", "24", "--num_gaussians", "40", "--seed", "1", "--device", "cpu", *extra]


def test_cli_weights_dir(fm, tmp_path, monkeypatch):
    from PIL import Image

    seen = {}
    real = fm.ViewShardedFitter

    def spy(*a, **kw):
        seen["weights"] = kw.get("weights")
        return real(*a, **kw)

    monkeypatch.setattr(fm, "ViewShardedFitter", spy)
    wdir = tmp_path / "w"
    wdir.mkdir()
    w0 = wref.weight_map(32, 24, RECT, 1).numpy()
    w1 = (np.arange(24 * 32).reshape(24, 32) % 256).astype(np.uint8)
    np.save(wdir / "v0.npy", w0)
    Image.fromarray(w1, mode="L").save(wdir / "v1.png")
    np.save(wdir / "v2.npy", np.full((24, 32), 2.0))  # float64: converted
    Image.fromarray(w1, mode="L").save(wdir / "v2.png")  # (the .npy wins)
    fm.main(_main_args(tmp_path / "a", "--weights_dir", str(wdir)))
    got = seen["weights"]
    assert len(got) == 3 and torch.equal(got[0], torch.from_numpy(w0))
    assert torch.equal(got[1], torch.from_numpy(w1.astype(np.float32) / 255.0)) and float(got[1].max()) == 1.0
    assert torch.equal(got[2].float(), torch.full((24, 32), 2.0))
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    # weights of ones: the fit without --weights_dir, the same files with the same contents
    ones = tmp_path / "ones"
    ones.mkdir()
    for k in range(3):
        np.save(ones / f"v{k}.npy", np.ones((24, 32), np.float32))
    fm.main(_main_args(tmp_path / "b", "--weights_dir", str(ones)))
    seen.clear()
    fm.main(_main_args(tmp_path / "c"))
    assert seen["weights"] is None
    assert sorted(p.name for p in (tmp_path / "b").iterdir()) == sorted(p.name for p in (tmp_path / "c").iterdir()) == files
    with np.load(tmp_path / "b" / "gaussians_fitted.npz") as x, np.load(tmp_path / "c" / "gaussians_fitted.npz") as y, \
            np.load(tmp_path / "a" / "gaussians_fitted.npz") as z:
        assert all(np.array_equal(x[k], y[k]) for k in y.files)
        assert not all(np.array_equal(z[k], y[k]) for k in y.files)
    assert (tmp_path / "b" / "loss.txt").read_text() == (tmp_path / "c" / "loss.txt").read_text()
    # held-out views need no file (view 0 is held out), and the training views keep their own
    (wdir / "v0.npy").unlink()
    fm.main(_main_args(tmp_path / "d", "--weights_dir", str(wdir), "--holdout_every", "3"))
    got = seen["weights"]
    assert len(got) == 2 and torch.equal(got[0], torch.from_numpy(w1.astype(np.float32) / 255.0))
    assert (tmp_path / "d" / "eval.json").exists()
