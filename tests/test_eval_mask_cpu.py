"""CPU: masked held-out metrics without a device.  losses.image_metrics_masked against the float64 restatement
(tests/eval_mask_reference.py), ViewShardedFitter.evaluate(masks=...) on host tensors (the composed route), its NaN and
mean rules and its validation errors, over two gloo ranks, the C entries' argument checks (before any launch) and
fit_multiview.main with --eval_masked.

Tolerances.  fg_fraction, fg_l1, fg_mse and sil_l1 are float32 element-wise terms summed in float64 against the same in
float64: VALUE_TOL, the project's bar for such a mean of values in [0, 1].  fg_ssim: VALUE_TOL for masks covering at least
10 % of the image (asserted): a float32 SSIM map differs from the float64 one by up to 4.9e-6 in single values but by at
most 2e-7 in masked means from 2 % coverage up, on random targets (as every case here has: where both images are flat and
equal, a float32 map cancels, which is tests/test_ssim_cpu.py's subject, not this file's).  The IoU's two counts are
exact (comparisons of the same float32 values)."""
from __future__ import annotations

import ctypes
import importlib
import json
import math
import multiprocessing as mp
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist

import eval_mask_reference as emr
import ssim_reference as ref
from conftest import GOLDEN, REPO

HERE = os.path.dirname(os.path.abspath(__file__))
W, H, V, N = 32, 24, 4, 80
FG = ("fg_l1", "fg_mse", "fg_psnr", "fg_ssim")
NEW = ("fg_fraction",) + FG + ("sil_l1", "sil_iou")


@pytest.fixture(scope="module")
def fm(pkg):
    return importlib.import_module("3dgaussian_amd.fit_multiview")


def _rand(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed))


def _check(losses, x, a, t, m, tag):
    got = losses.image_metrics_masked(x, a, t, m)
    want = emr.metrics(x, a, t, m)
    print(f"masked {tag}: " + " ".join(f"{k} {float(got[k]):.8f} (f64 {want[k]:.8f})" for k in emr.KEYS))
    assert sorted(got) == sorted(NEW)
    assert want["fg_fraction"] >= 0.1  # the condition of fg_ssim's bar
    for k in ("fg_fraction", "fg_l1", "fg_mse", "fg_ssim", "sil_l1"):
        assert abs(float(got[k]) - want[k]) <= ref.VALUE_TOL, k
    assert float(got["sil_iou"]) == want["sil_iou"]
    assert float(got["fg_psnr"]) == float(-10.0 * torch.log10(got["fg_mse"]))
    return got, want


@pytest.mark.parametrize("soft", [False, True], ids=["binary", "soft"])
@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("shape", [(64, 48, 3), (37, 50, 3), (15, 17, 3), (5, 7, 3), (1, 1, 3)])
def test_composed_route_matches_float64(pkg, shape, kind, soft):
    x, t = ref.inputs(kind, shape)[0], _rand(shape, 11)  # (noise or blobs on black, against a random target)
    Hh, Ww = shape[:2]
    a = _rand((Hh, Ww), 31)
    a[0, 0] = 0.5  # exactly the threshold: not above
    m = emr.blob_mask(Hh, Ww, soft)
    assert bool((m == 0.5).any())
    got, want = _check(pkg.losses, x, a, t, m, f"{kind} {shape} {'soft' if soft else 'binary'}")
    assert want["union"] >= want["inter"] and (want["union"] > 0 or Hh * Ww == 1)


def test_mask_of_ones_is_the_whole_image(pkg):
    x, t = ref.inputs("render", (64, 48, 3))[0], _rand((64, 48, 3), 11)
    got, _ = _check(pkg.losses, x, torch.ones((64, 48)), t, torch.ones((64, 48)), "ones")
    plain = pkg.losses.image_metrics(x, t)
    assert float(got["fg_fraction"]) == 1.0 and float(got["sil_l1"]) == 0.0 and float(got["sil_iou"]) == 1.0
    for k in ("l1", "mse"):
        assert abs(float(got["fg_" + k]) - float(plain[k])) <= ref.VALUE_TOL


def test_empty_mask_and_empty_union(pkg):
    x, t = ref.inputs("uniform", (15, 17, 3))
    a = _rand((15, 17), 2)
    got = pkg.losses.image_metrics_masked(x, a, t, torch.zeros((15, 17)))
    want = emr.metrics(x, a, t, torch.zeros((15, 17)))
    assert float(got["fg_fraction"]) == 0.0 and all(math.isnan(float(got[k])) and math.isnan(want[k]) for k in FG)
    assert abs(float(got["sil_l1"]) - float(a.double().mean())) <= ref.VALUE_TOL
    assert float(got["sil_iou"]) == 0.0 == want["sil_iou"] and want["inter"] == 0 and want["union"] > 0
    both = pkg.losses.image_metrics_masked(x, torch.full((15, 17), 0.5), t, torch.full((15, 17), 0.5))
    assert float(both["sil_iou"]) == 1.0 and float(both["sil_l1"]) == 0.0  # 0.5 is not above: an empty union
    for bad in ((x, a[:-1], t, a), (x, a, t, a[:, :-1]), (x[:, :, :2], a, t[:, :, :2], a), (x, a, t[:-1], a)):
        with pytest.raises(ValueError):
            pkg.losses.image_metrics_masked(*bad)


# ---- the fitter on host tensors ----------------------------------------------------------------------------------------
def _masks():
    return [emr.blob_mask(H, W, soft=bool(i % 2), seed=i) for i in range(V)]


def _fitter(fm, masks=True, **kw):
    torch.manual_seed(5)
    dev = torch.device("cpu")
    params = fm.build_params(N, dev, use_sh=False)
    with torch.no_grad():
        params["scales_raw"].fill_(-1.0)
        params["colors_raw"].add_(1.0)
    cams = fm.orbit_cameras(V, W, H, dev)
    targets = [_rand((H, W, 3), 20 + i) for i in range(V)]
    return fm.ViewShardedFitter(params, cams, targets, W, H, masks=_masks() if masks else None, **kw), cams, targets


def _render(pkg, fm, fit, cam):
    with torch.no_grad():
        m, s, c, o = fm.activations(fit.params)
        return pkg.cpu_renderer.render(m, s, c, o, cam.view, cam.proj, W, H, torch.zeros(3))[:2]


def test_evaluate_on_host_tensors(pkg, fm):
    fit, cams, targets = _fitter(fm)
    fit.step()
    plain = fit.evaluate()
    masks = _masks()
    got = fit.evaluate(masks=masks)
    assert sorted(got) == sorted(list(plain) + list(NEW) + ["mean_" + k for k in NEW])
    for k in plain:  # the plain keys: the same bits as without the argument
        assert np.array_equal(np.asarray(got[k]), np.asarray(plain[k])), k
    for i, (cam, t) in enumerate(zip(cams, targets)):
        img, alpha = _render(pkg, fm, fit, cam)
        want = emr.metrics(img, alpha, t, masks[i])
        assert want["fg_fraction"] >= 0.1
        for k in ("fg_fraction", "fg_l1", "fg_mse", "fg_ssim", "sil_l1"):
            assert abs(got[k][i] - want[k]) <= ref.VALUE_TOL, (k, i)
        assert abs(got["sil_iou"][i] - want["sil_iou"]) <= 1e-7  # (the ratio of the exact counts, through a float32)
        assert got["fg_psnr"][i] == -10.0 * np.log10(got["fg_mse"][i])
    for k in NEW:
        assert got[k].dtype == np.float64 and got["mean_" + k] == float(got[k].mean()), k
    same = fit.evaluate(masks=True)
    for k in got:
        assert np.array_equal(np.asarray(same[k]), np.asarray(got[k])), k
    sub = fit.evaluate([cams[2], cams[0]], [targets[2], targets[0]], masks=[masks[2], masks[0]])
    for k in NEW + ("psnr",):
        assert sub[k].tolist() == [got[k][2], got[k][0]], k
    both = fit.evaluate(masks=masks, color_correct=True)
    cc = fit.evaluate(color_correct=True)
    for k in got:
        assert np.array_equal(np.asarray(both[k]), np.asarray(got[k])), k
    for k in cc:
        assert np.array_equal(np.asarray(both[k]), np.asarray(cc[k])), k


def test_empty_masks_and_the_means(pkg, fm):
    fit, cams, targets = _fitter(fm)
    masks = _masks()
    masks[1] = torch.zeros((H, W))
    got = fit.evaluate(masks=masks)
    some = [0, 2, 3]
    assert got["fg_fraction"][1] == 0.0 and all(math.isnan(got[k][1]) for k in FG)
    for k in FG:
        assert np.isfinite(got[k][some]).all() and got["mean_" + k] == float(got[k][some].mean()), k
    for k in ("fg_fraction", "sil_l1", "sil_iou"):
        assert np.isfinite(got[k]).all() and got["mean_" + k] == float(got[k].mean()), k
    _, alpha = _render(pkg, fm, fit, cams[1])
    assert abs(got["sil_l1"][1] - float(alpha.double().mean())) <= ref.VALUE_TOL
    none = fit.evaluate(masks=[torch.zeros((H, W))] * V)
    assert all(math.isnan(none["mean_" + k]) for k in FG) and math.isfinite(none["mean_sil_l1"])
    assert math.isfinite(none["mean_psnr"])


def test_validation_errors(fm):
    fit, cams, targets = _fitter(fm)
    masks = _masks()
    with pytest.raises(ValueError, match="one .* mask per view"):
        fit.evaluate(masks=masks[:-1])
    with pytest.raises(ValueError, match="mask is a"):
        fit.evaluate(masks=masks[:-1] + [torch.zeros((H, W + 1))])
    with pytest.raises(ValueError, match="mask is a"):
        fit.evaluate(masks=masks[:-1] + [None])
    with pytest.raises(ValueError, match="masks=True"):
        fit.evaluate([cams[0]], [targets[0]], masks=True)
    bare, _, _ = _fitter(fm, masks=False)
    with pytest.raises(ValueError, match="no masks"):
        bare.evaluate(masks=True)
    assert "fg_l1" in bare.evaluate(masks=masks)  # (a fitter without masks of its own evaluates against given ones)


def test_evaluate_masked_does_not_change_the_fit(fm):
    a, _, _ = _fitter(fm)
    b, _, _ = _fitter(fm)
    la = [a.step() for _ in range(3)]
    lb = [b.step()]
    rng = torch.get_rng_state()
    b.evaluate(masks=True)
    assert torch.equal(rng, torch.get_rng_state())
    lb += [b.step() for _ in range(2)]
    for x, y in zip(la, lb):
        assert torch.equal(x, y)
    for k in a.params:
        assert torch.equal(a.params[k], b.params[k]), k


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, REPO)
    sys.path.insert(0, HERE)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    fm = importlib.import_module("3dgaussian_amd.fit_multiview")
    fit, _, _ = _fitter(fm)
    masks = _masks()
    masks[1] = torch.zeros((H, W))
    r = fit.evaluate(masks=masks)
    out_q.put((rank, {k: np.asarray(v).copy() for k, v in r.items()}))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_gloo_ranks_return_the_single_process_dict(fm):
    fit, _, _ = _fitter(fm)
    masks = _masks()
    masks[1] = torch.zeros((H, W))
    want = fit.evaluate(masks=masks)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=240) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for k in want:
        for r in (0, 1):
            assert np.array_equal(res[r][k], np.asarray(want[k]), equal_nan=True), (k, r)


def test_abi_argument_checks(pkg):
    """gr_eval_mask_ws_bytes and the checks of gr_eval_view_masked / gr_eval_views_masked that come before any launch
    (pointers never read)."""
    nat = pkg._native
    L = nat.lib()
    header = open(os.path.join(REPO, "include", "gr_hip.h")).read()
    assert "#define GR_EVAL_MASK_METRICS 6" in header and nat.EVAL_MASK_METRICS == 6 == len(emr.KEYS)
    fmod = importlib.import_module("3dgaussian_amd.fit_multiview")
    assert fmod.MASK_KEYS == emr.KEYS
    gv = pkg.torch_renderer.make_view(np.eye(4, dtype="float32"), np.eye(4, dtype="float32"), 50, 37, depth_grad=False)
    need, need_eval = L.gr_eval_mask_ws_bytes(ctypes.byref(gv)), L.gr_eval_ws_bytes(ctypes.byref(gv))
    assert need >= 7 * 4 * 12 and 3 * need == 7 * need_eval  # seven planes to gr_eval_view's three
    buf = (ctypes.c_float * 8)()
    p, null = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(0)
    call = lambda v, saved=p, target=p, mask=p, out=p, ws=p, nb=need: L.gr_eval_view_masked(  # noqa: E731
        ctypes.byref(v), saved, target, mask, out, ws, nb, null)
    assert call(gv, nb=need - 1) == nat.GR_ERR_WORKSPACE
    assert b"gr_eval_view_masked" in L.gr_last_error() and b"workspace" in L.gr_last_error()
    for kw in (dict(saved=null), dict(target=null), dict(mask=null), dict(out=null), dict(ws=null)):
        assert call(gv, **kw) == nat.GR_ERR_INVALID_ARGUMENT, kw
    for field, value in (("tile", 32), ("rows", 1)):
        bad = nat.GrView.from_buffer_copy(gv)
        setattr(bad, field, value)
        assert call(bad) == nat.GR_ERR_INVALID_ARGUMENT
    tall = nat.GrView.from_buffer_copy(gv)
    tall.width, tall.height = 1, 16 * 65535 + 1
    assert L.gr_eval_mask_ws_bytes(ctypes.byref(tall)) == 0 and call(tall) == nat.GR_ERR_INVALID_ARGUMENT
    cfg = nat.GrFitConfig(1, 1, 1, 1, 0, 0)
    tgt = (nat.GrFitTarget * 1)()
    views = lambda ex, nv, arr, n: L.gr_eval_views_masked(ex, ctypes.byref(cfg), nv, arr, n, p, p, p, 3, p, p, null)  # noqa: E731
    assert views(null, 1, None, 10) == nat.GR_ERR_INVALID_ARGUMENT
    tgt[0].target_rgb = ctypes.addressof(buf)
    tgt[0].target_mask = None
    assert views(p, 1, tgt, 10) == nat.GR_ERR_INVALID_ARGUMENT and b"null mask" in L.gr_last_error()
    caps = (nat.GrPlan * 1)()
    cfg.caps = caps
    assert views(p, 1, tgt, 10) == nat.GR_ERR_INVALID_ARGUMENT and b"caps" in L.gr_last_error()
    cfg.caps = None
    assert views(p, 0, None, 10) == nat.GR_OK and views(p, 1, tgt, 0) == nat.GR_OK  # no views, no Gaussians: no-ops
    assert callable(pkg.torch_renderer.eval_view_masked_native)


# ---- the command line ------------------------------------------------------------------------------------------------
def _main_args(out_dir, *extra):
    return ["--targets_dir", os.path.join(GOLDEN, "fit_targets"), "--out_dir", str(out_dir), "--iters", "2", "--width", "32",
            "--height", "32", "--num_gaussians", "60", "--seed", "1", "--device", "cpu", "--holdout_every", "2", *extra]


def _write_masks(fm, mdir, args_thresh=0.06):
    """One mask per target: the threshold rule's for v1 and v2, for the held-out v0 a square that the rule would never
    give.  Returns the masks as main() will load them."""
    from PIL import Image

    mdir.mkdir()
    out = {}
    for stem in ("v0", "v1", "v2"):
        t = torch.from_numpy(fm._load_image(os.path.join(GOLDEN, "fit_targets", stem + ".png"), 32, 32))
        m = (t.mean(dim=2) > args_thresh).to(torch.uint8) * 255
        if stem == "v0":
            m = torch.zeros((32, 32), dtype=torch.uint8)
            m[2:12, 3:9] = 255
        Image.fromarray(m.numpy(), mode="L").save(mdir / (stem + ".png"))
        out[stem] = m.float() / 255.0
    return out


def test_cli_eval_masked(fm, tmp_path, capsys):
    masks = _write_masks(fm, tmp_path / "masks")
    plain, masked = tmp_path / "plain", tmp_path / "masked"
    fm.main(_main_args(plain, "--masks_dir", str(tmp_path / "masks")))
    out_plain = capsys.readouterr().out
    fm.main(_main_args(masked, "--masks_dir", str(tmp_path / "masks"), "--eval_masked"))
    out_masked = capsys.readouterr().out
    a, b = json.loads((plain / "eval.json").read_text()), json.loads((masked / "eval.json").read_text())
    assert len(a) == len(b) == 1 and a[0]["views"] == b[0]["views"] == [0, 2]
    assert sorted(a[0]) == ["iter", "l1", "mean_l1", "mean_psnr", "mean_ssim", "n", "psnr", "ssim", "views"]  # as before
    new = ["fg_fraction", "fg_l1", "fg_psnr", "fg_ssim", "sil_iou", "sil_l1"]
    assert sorted(set(b[0]) - set(a[0])) == sorted(new + ["mean_" + k for k in new])
    for k in a[0]:
        assert a[0][k] == b[0][k], k  # the plain values are the same with the flag
    e = b[0]
    # the held-out views' own masks: v0's square (60 pixels, not the threshold rule's), v2's as written
    assert e["fg_fraction"] == [float(masks["v0"].mean()), float(masks["v2"].mean())] and e["fg_fraction"][0] == 60 / 1024
    rule = (torch.from_numpy(fm._load_image(os.path.join(GOLDEN, "fit_targets", "v0.png"), 32, 32)).mean(dim=2) > 0.06).float()
    assert float(rule.mean()) != e["fg_fraction"][0]
    for k in new:
        assert len(e[k]) == 2 and all(math.isfinite(x) for x in e[k]) and e["mean_" + k] == float(np.mean(e[k])), k
    assert "masked:" not in out_plain and out_plain.count("eval iter") == 1
    assert out_masked.count("masked:") == 1 and out_masked.count("eval iter") == 2
    for name in ("gaussians_fitted.npz", "loss.txt", "preview_view0.png"):
        assert (plain / name).read_bytes() == (masked / name).read_bytes(), name
    # the threshold rule's masks (--silhouette_weight > 0, no --masks_dir) serve too; no masks at all is an error
    fm.main(_main_args(tmp_path / "rule", "--eval_masked"))
    r = json.loads((tmp_path / "rule" / "eval.json").read_text())[0]
    assert r["fg_fraction"][0] == float(rule.mean())
    with pytest.raises(ValueError, match="--eval_masked needs masks"):
        fm.main(_main_args(tmp_path / "none", "--eval_masked", "--silhouette_weight", "0"))
