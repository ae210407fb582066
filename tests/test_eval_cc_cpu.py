"""CPU: colour-corrected held-out metrics without a device.  losses.color_correct / apply_color_transform /
image_metrics_cc against the float64 numpy restatement (tests/cc_reference.py), ViewShardedFitter.evaluate(color_correct=
True) on host tensors (the composed route), the C entries' argument checks (before any launch) and fit_multiview.main with
--eval_color_correct.

Tolerances.  A transform against the reference's: both are float64 Cholesky solves of the same 4 x 4 system, rounded to
float32 once; their moments differ by the order of a float64 sum (1e-16 relative), which the ridge amplifies by at most
1 / ridge = 1e6 in a rank-deficient direction (1e-9, include/gr_hip.h), so they agree to a float32 rounding of an entry of
magnitude <= 2 (2.4e-7): E_TOL = 1e-6.  l1 and mse against a float64 evaluation with the same transform: VALUE_TOL, the
project's bar for a float32 mean of values in [0, 1] (the float32 apply moves a value by a few 1e-7 at most, a mean by
less).  ssim: VALUE_TOL plus the error of the dense float32 evaluation on the same images, as tests/test_eval_cpu.py."""
from __future__ import annotations

import ctypes
import importlib
import json
import math
import os

import numpy as np
import pytest
import torch

import cc_reference as cc
import ssim_reference as ref
from conftest import GOLDEN, REPO

E_TOL = 1e-6
W, H, V, N = 32, 24, 4, 80


@pytest.fixture(scope="module")
def fm(pkg):
    return importlib.import_module("3dgaussian_amd.fit_multiview")


def _rand(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed))


def _ssim_tol(y, t) -> float:
    """VALUE_TOL + the dense float32 evaluation's own error on (y, t)."""
    y, t = torch.as_tensor(y), torch.as_tensor(t)
    return ref.VALUE_TOL + abs(float(ref.dssim_dense(y.float(), t.float())) - float(ref.dssim_dense(y.double(), t.double())))


def _check_against_reference(losses, x, t, tag):
    """image_metrics_cc(x, t) against cc_reference: the transform, then the corrected metrics of that transform."""
    got = losses.image_metrics_cc(x, t)
    E = got["cc_transform"]
    assert E.shape == (3, 4) and E.dtype == torch.float32
    want_E = cc.fit(x, t)
    err = float(np.abs(E.numpy().astype(np.float64) - want_E).max())
    want = cc.metrics(x, t, E)
    print(f"cc {tag}: |E - ref| {err:.2e}; cc_l1 {float(got['cc_l1']):.8f} (f64 {want['l1']:.8f}) cc_mse "
          f"{float(got['cc_mse']):.8f} (f64 {want['mse']:.8f}) cc_ssim {float(got['cc_ssim']):.8f} (f64 {want['ssim']:.8f})")
    assert np.isfinite(E.numpy()).all() and err <= E_TOL
    assert abs(float(got["cc_l1"]) - want["l1"]) <= ref.VALUE_TOL
    assert abs(float(got["cc_mse"]) - want["mse"]) <= ref.VALUE_TOL
    assert abs(float(got["cc_ssim"]) - want["ssim"]) <= _ssim_tol(cc.apply(x, E), t)
    assert float(got["cc_psnr"]) == float(-10.0 * torch.log10(got["cc_mse"]))
    plain = losses.image_metrics(x, t)
    for k in plain:
        assert torch.equal(got[k], plain[k]), k
    return got


def test_recovers_a_known_gain_and_offset(pkg):
    """t = E0 (x, 1) with gains and offsets that keep it inside [0, 1], x full-rank uniform noise at 32 x 24 (the
    smallest eigenvalue of its moment matrix A / HW is about the channel variance 1 / 12 = 0.08): the ridge pulls the
    solution by about ridge / 0.08 = 1.2e-5 times |E0 - I| < 1: within 1e-4."""
    losses = pkg.losses
    x = _rand((H, W, 3), 3)
    E0 = torch.tensor([[0.8, 0.0, 0.0, 0.03], [0.0, 0.7, 0.0, 0.1], [0.0, 0.0, 0.9, 0.05]])
    t = losses.apply_color_transform(x, E0)
    assert float(t.min()) >= 0.0 and float(t.max()) <= 1.0
    A, _ = cc.moments(x, t)
    lo = float(np.linalg.eigvalsh(A / (H * W)).min())
    E = losses.color_correct(x, t)
    err = float((E - E0).abs().max())
    print(f"recovery: smallest moment eigenvalue {lo:.4f}, |E - E0| {err:.2e}")
    assert 0.04 < lo < 0.12 and err <= 1e-4
    got = _check_against_reference(losses, x, t, "gain/offset")
    assert float(got["cc_mse"]) <= 1e-8 and float(got["mse"]) > 1e-3
    # the apply is the element-wise float32 form, in the stated order
    y = losses.apply_color_transform(x, E)
    e = E.numpy()
    xn = x.numpy()
    for k in range(3):
        want = ((np.float32(e[k, 0]) * xn[..., 0] + np.float32(e[k, 1]) * xn[..., 1]) + np.float32(e[k, 2]) * xn[..., 2]) \
            + np.float32(e[k, 3])
        assert np.array_equal(y[..., k].numpy(), want.astype(np.float32))
    assert torch.equal(losses.apply_color_transform(x, E.reshape(12)), y)
    for bad in (0.0, -1e-6, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            losses.color_correct(x, t, bad)
    with pytest.raises(ValueError):
        losses.color_correct(x, t[:-1])


@pytest.mark.parametrize("shape", [(H, W, 3), (5, 7, 3), (1, 1, 3)])
def test_target_equal_to_the_image(pkg, shape):
    losses = pkg.losses
    x = _rand(shape, 5)
    got = losses.image_metrics_cc(x, x.clone())
    err = float(np.abs(got["cc_transform"].numpy() - cc.IDENTITY).max())
    print(f"target = image {shape}: |E - [I | 0]| {err:.2e}")
    assert err <= 1e-6
    for k in ("l1", "mse", "ssim"):
        assert abs(float(got["cc_" + k]) - float(got[k])) <= ref.VALUE_TOL, k


@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("shape", [(64, 48, 3), (15, 17, 3), (5, 7, 3)])
def test_corrected_is_never_worse(pkg, kind, shape):
    """The identity is feasible, so in exact arithmetic cc_mse <= mse; in float32 within VALUE_TOL."""
    x, t = ref.inputs(kind, shape)
    got = _check_against_reference(pkg.losses, x, t, f"{kind} {shape}")
    assert float(got["cc_mse"]) <= float(got["mse"]) + ref.VALUE_TOL


@pytest.mark.parametrize("case", ["grey", "constant", "1x1", "1x1 black"])
def test_degenerate_images(pkg, case):
    """Rank 2 (equal channels), rank 1 (one colour) and one pixel: the ridge keeps them defined."""
    if case == "grey":
        x = _rand((H, W, 1), 7).expand(H, W, 3).contiguous()
        t = _rand((H, W, 3), 8)
    elif case == "constant":
        x = torch.tensor([0.2, 0.5, 0.7]).expand(H, W, 3).contiguous()
        t = _rand((H, W, 3), 8)
    else:
        x = torch.zeros((1, 1, 3)) if "black" in case else torch.tensor([[[0.3, 0.6, 0.1]]])
        t = torch.tensor([[[0.9, 0.2, 0.4]]])
    got = _check_against_reference(pkg.losses, x, t, case)
    for k in ("cc_l1", "cc_mse", "cc_psnr", "cc_ssim"):
        assert math.isfinite(float(got[k])) or (k == "cc_psnr" and float(got["cc_mse"]) == 0.0), k
    assert float(got["cc_mse"]) <= float(got["mse"]) + ref.VALUE_TOL


# ---- the fitter on host tensors ----------------------------------------------------------------------------------------
def _fitter(fm, **kw):
    torch.manual_seed(5)
    dev = torch.device("cpu")
    params = fm.build_params(N, dev, use_sh=False)
    with torch.no_grad():
        params["scales_raw"].fill_(-1.0)
        params["colors_raw"].add_(1.0)
    cams = fm.orbit_cameras(V, W, H, dev)
    targets = [_rand((H, W, 3), 20 + i) for i in range(V)]
    return fm.ViewShardedFitter(params, cams, targets, W, H, **kw), cams, targets


def _render(pkg, fm, fit, cam):
    with torch.no_grad():
        m, s, c, o = fm.activations(fit.params)
        return pkg.cpu_renderer.render(m, s, c, o, cam.view, cam.proj, W, H, torch.zeros(3))[0]


def test_evaluate_on_host_tensors(pkg, fm):
    fit, cams, targets = _fitter(fm)
    fit.step()
    plain = fit.evaluate()
    got = fit.evaluate(color_correct=True)
    assert sorted(got) == sorted(list(plain) + ["cc_l1", "cc_mse", "cc_psnr", "cc_ssim", "cc_transform", "mean_cc_l1",
                                                "mean_cc_mse", "mean_cc_psnr", "mean_cc_ssim"])
    for k in plain:  # the plain keys: the same bits as without the argument
        assert np.array_equal(np.asarray(got[k]), np.asarray(plain[k])), k
    assert got["cc_transform"].shape == (V, 3, 4) and got["cc_transform"].dtype == np.float64
    for i, (cam, t) in enumerate(zip(cams, targets)):
        img = _render(pkg, fm, fit, cam)
        E = got["cc_transform"][i]
        assert np.abs(E - cc.fit(img, t)).max() <= E_TOL
        assert np.array_equal(E.astype(np.float32).astype(np.float64), E)  # float32 values
        want = cc.metrics(img, t, E)
        assert abs(got["cc_l1"][i] - want["l1"]) <= ref.VALUE_TOL
        assert abs(got["cc_mse"][i] - want["mse"]) <= ref.VALUE_TOL
        assert abs(got["cc_ssim"][i] - want["ssim"]) <= _ssim_tol(cc.apply(img, E), t)
        assert got["cc_psnr"][i] == -10.0 * np.log10(got["cc_mse"][i])
        assert got["cc_mse"][i] <= got["mse"][i] + ref.VALUE_TOL
        comp = pkg.losses.image_metrics_cc(img, t)
        for k in ("l1", "mse", "ssim"):
            assert got["cc_" + k][i] == float(comp["cc_" + k]), (k, i)
    for k in ("l1", "mse", "psnr", "ssim"):
        assert got["mean_cc_" + k] == float(got["cc_" + k].mean()) and got["cc_" + k].dtype == np.float64
    sub = fit.evaluate([cams[2], cams[0]], [targets[2], targets[0]], color_correct=True)
    assert np.array_equal(sub["cc_transform"], got["cc_transform"][[2, 0]])
    assert sub["cc_mse"].tolist() == [got["cc_mse"][2], got["cc_mse"][0]]
    # another ridge is another transform; a ridge that is not positive and finite is refused
    assert not np.array_equal(fit.evaluate(color_correct=True, ridge=1e-2)["cc_transform"], got["cc_transform"])
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            fit.evaluate(color_correct=True, ridge=bad)


def test_held_out_view_with_a_gain(pkg, fm):
    """The Gaussians are exact, the held-out photo is 0.8 x + 0.03: the plain PSNR is poor, the corrected error none."""
    fit, cams, _ = _fitter(fm)
    held = fm.orbit_cameras(V + 1, W, H, torch.device("cpu"))[2]
    img = _render(pkg, fm, fit, held)
    assert float(img.std()) > 0.05  # (a view with content)
    r = fit.evaluate([held], [0.8 * img + 0.03], color_correct=True)
    print(f"held-out gain: psnr {r['psnr'][0]:.2f} dB, cc_psnr {r['cc_psnr'][0]:.2f} dB, cc_mse {r['cc_mse'][0]:.3e}, E "
          f"{r['cc_transform'][0].round(5).tolist()}")
    assert r["psnr"][0] < 35.0 and r["mse"][0] > 1e-4
    assert r["cc_mse"][0] < 1e-8 and r["cc_ssim"][0] > 1.0 - 1e-4


def test_evaluate_cc_does_not_change_the_fit(fm):
    a, _, _ = _fitter(fm)
    b, _, _ = _fitter(fm)
    la = [a.step() for _ in range(3)]
    lb = [b.step()]
    rng = torch.get_rng_state()
    b.evaluate(color_correct=True)
    assert torch.equal(rng, torch.get_rng_state())
    lb += [b.step() for _ in range(2)]
    for x, y in zip(la, lb):
        assert torch.equal(x, y)
    for k in a.params:
        assert torch.equal(a.params[k], b.params[k]), k


def test_abi_argument_checks(pkg):
    """gr_cc_ws_bytes and the checks of gr_cc_fit_view / gr_eval_view_cc / gr_eval_views_cc that come before any launch
    (pointers never read)."""
    nat = pkg._native
    L = nat.lib()
    header = open(os.path.join(REPO, "include", "gr_hip.h")).read()
    for name, value in (("GR_CC_MOMENTS", nat.CC_MOMENTS), ("GR_CC_TRANSFORM", nat.CC_TRANSFORM),
                        ("GR_EVAL_CC_ROW", nat.EVAL_CC_ROW)):
        assert f"#define {name} {value}" in header
    assert (nat.CC_MOMENTS, nat.CC_TRANSFORM, nat.EVAL_CC_ROW) == (22, 12, 18) and "#define GR_CC_RIDGE 1e-6f" in header
    assert nat.CC_RIDGE == pkg.losses.CC_RIDGE == cc.RIDGE
    gv = pkg.torch_renderer.make_view(np.eye(4, dtype="float32"), np.eye(4, dtype="float32"), 50, 37, depth_grad=False)
    need, need_eval = L.gr_cc_ws_bytes(ctypes.byref(gv)), L.gr_eval_ws_bytes(ctypes.byref(gv))
    assert need >= 22 * 8 * 4 * 3
    buf = (ctypes.c_float * 4)()
    p, null = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(0)
    ridge = ctypes.c_float(1e-6)
    assert L.gr_cc_fit_view(ctypes.byref(gv), p, p, ridge, p, p, need - 1, null) == nat.GR_ERR_WORKSPACE
    assert b"gr_cc_fit_view" in L.gr_last_error() and b"workspace" in L.gr_last_error()
    assert L.gr_eval_view_cc(ctypes.byref(gv), p, p, p, p, p, need_eval - 1, null) == nat.GR_ERR_WORKSPACE
    for args in ((null, p, p, p), (p, null, p, p), (p, p, null, p), (p, p, p, null)):
        saved, target, out, ws = args
        assert L.gr_cc_fit_view(ctypes.byref(gv), saved, target, ridge, out, ws, need, null) == nat.GR_ERR_INVALID_ARGUMENT
        assert L.gr_eval_view_cc(ctypes.byref(gv), saved, target, p, out, ws, need_eval, null) == nat.GR_ERR_INVALID_ARGUMENT
    assert L.gr_eval_view_cc(ctypes.byref(gv), p, p, null, p, p, need_eval, null) == nat.GR_ERR_INVALID_ARGUMENT
    for bad in (0.0, -1e-6, float("inf"), float("nan")):
        assert L.gr_cc_fit_view(ctypes.byref(gv), p, p, ctypes.c_float(bad), p, p, need, null) == nat.GR_ERR_INVALID_ARGUMENT
        assert b"ridge" in L.gr_last_error()
    for field, value in (("tile", 32), ("rows", 1)):
        bad = nat.GrView.from_buffer_copy(gv)
        setattr(bad, field, value)
        assert L.gr_cc_fit_view(ctypes.byref(bad), p, p, ridge, p, p, need, null) == nat.GR_ERR_INVALID_ARGUMENT
        assert L.gr_eval_view_cc(ctypes.byref(bad), p, p, p, p, p, need_eval, null) == nat.GR_ERR_INVALID_ARGUMENT
    tall = nat.GrView.from_buffer_copy(gv)
    tall.width, tall.height = 1, 16 * 65535 + 1
    assert L.gr_cc_ws_bytes(ctypes.byref(tall)) == 0
    assert L.gr_cc_fit_view(ctypes.byref(tall), p, p, ridge, p, p, need, null) == nat.GR_ERR_INVALID_ARGUMENT
    cfg = nat.GrFitConfig(1, 1, 1, 1, 0, 0)
    tgt = (nat.GrFitTarget * 1)()
    call = lambda ex, nv, views, n, r=ridge: L.gr_eval_views_cc(ex, ctypes.byref(cfg), nv, views, n, p, p, p, 3, p, r, p, null)  # noqa: E731
    assert call(null, 1, None, 10) == nat.GR_ERR_INVALID_ARGUMENT
    assert call(p, 1, tgt, 10, ctypes.c_float(0.0)) == nat.GR_ERR_INVALID_ARGUMENT and b"ridge" in L.gr_last_error()
    assert call(p, 1, tgt, 10, ctypes.c_float(float("nan"))) == nat.GR_ERR_INVALID_ARGUMENT
    caps = (nat.GrPlan * 1)()
    cfg.caps = caps
    assert call(p, 1, tgt, 10) == nat.GR_ERR_INVALID_ARGUMENT and b"caps" in L.gr_last_error()
    cfg.caps = None
    assert call(p, 0, None, 10) == nat.GR_OK and call(p, 1, tgt, 0) == nat.GR_OK  # no views, no Gaussians: no-ops
    assert callable(pkg.torch_renderer.cc_fit_view_native) and callable(pkg.torch_renderer.eval_view_cc_native)


# ---- the command line ------------------------------------------------------------------------------------------------
def _main_args(tmp_path, *extra):
    return ["--targets_dir", os.path.join(GOLDEN, "fit_targets"), "--out_dir", str(tmp_path), "--iters", "2", "--width", "32",
            "--height", "32", "--num_gaussians", "60", "--seed", "1", "--device", "cpu", "--holdout_every", "2", *extra]


def test_cli_eval_color_correct(fm, tmp_path, capsys):
    plain, corr = tmp_path / "plain", tmp_path / "cc"
    fm.main(_main_args(plain))
    out_plain = capsys.readouterr().out
    fm.main(_main_args(corr, "--eval_color_correct", "--eval_ridge", "1e-5"))
    out_cc = capsys.readouterr().out
    a, b = json.loads((plain / "eval.json").read_text()), json.loads((corr / "eval.json").read_text())
    assert len(a) == len(b) == 1 and a[0]["views"] == b[0]["views"] == [0, 2]
    assert not [k for k in a[0] if "cc_" in k] and "colour-corrected" not in out_plain
    assert sorted(set(b[0]) - set(a[0])) == ["cc_l1", "cc_psnr", "cc_ssim", "cc_transform", "mean_cc_l1", "mean_cc_psnr",
                                             "mean_cc_ssim"]
    for k in a[0]:
        assert a[0][k] == b[0][k], k  # the plain values are the same with the flag
    e = b[0]
    assert np.asarray(e["cc_transform"]).shape == (2, 3, 4)
    for k in ("psnr", "ssim", "l1"):
        assert len(e["cc_" + k]) == 2 and all(math.isfinite(x) for x in e["cc_" + k])
        assert e["mean_cc_" + k] == float(np.mean(e["cc_" + k]))
    assert all(c >= p - 1e-3 for c, p in zip(e["cc_psnr"], e["psnr"]))  # (corrected never worse, up to rounding)
    assert out_cc.count("colour-corrected") == 1 and out_cc.count("eval iter") == 2
    for name in ("gaussians_fitted.npz", "loss.txt", "preview_view0.png"):
        assert (plain / name).read_bytes() == (corr / name).read_bytes(), name
