"""CPU: held-out evaluation without a device: losses.psnr / losses.image_metrics against float64 numpy,
ViewShardedFitter.evaluate on host tensors (the composed route through cpu_renderer), over two gloo ranks, the C entries'
argument checks (before any launch) and fit_multiview.main with --holdout_every / --eval_interval."""
from __future__ import annotations

import ctypes
import importlib
import json
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import ssim_reference as ref
from conftest import GOLDEN, REPO

HERE = os.path.dirname(os.path.abspath(__file__))
W = H = 32
N = 60


@pytest.fixture(scope="module")
def fm(pkg):
    return importlib.import_module("3dgaussian_amd.fit_multiview")


@pytest.mark.parametrize("shape", [(64, 48, 3), (5, 7, 3)])
def test_metrics_match_float64(pkg, shape):
    """l1, mse, psnr of float32 torch means against numpy float64 on the same inputs: a float32 mean of values in [0, 1]
    is within VALUE_TOL (the project's bar for such a sum); psnr = -10 log10 mse then moves by (10 / ln 10) d mse / mse;
    ssim against the dense float64 reference within VALUE_TOL plus the float32 dense evaluation's own error."""
    losses = pkg.losses
    x, y = ref.inputs("render", shape)
    m = losses.image_metrics(x, y)
    xd, yd = x.double().numpy(), y.double().numpy()
    l1, mse = np.abs(xd - yd).mean(), ((xd - yd) ** 2).mean()
    assert abs(float(m["l1"]) - l1) <= ref.VALUE_TOL
    assert abs(float(m["mse"]) - mse) <= ref.VALUE_TOL
    tol_db = (10.0 / math.log(10.0)) * ref.VALUE_TOL / mse + 1e-5
    assert abs(float(m["psnr"]) - (-10.0 * math.log10(mse))) <= tol_db
    assert abs(float(losses.psnr(x, y)) - float(m["psnr"])) == 0.0
    want = 1.0 - float(ref.dssim_dense(x.double(), y.double()))
    assert abs(float(m["ssim"]) - want) <= ref.VALUE_TOL + ref.reference("render", shape)["v32"]
    same = losses.image_metrics(x, x)
    assert float(same["l1"]) == 0.0 and float(same["mse"]) == 0.0 and math.isinf(float(same["psnr"])) and float(same["psnr"]) > 0
    assert math.isinf(float(losses.psnr(y, y)))
    with pytest.raises(ValueError):
        losses.psnr(x, y[:-1])


def test_abi_argument_checks(pkg):
    """gr_eval_ws_bytes and gr_eval_view / gr_eval_views' checks that come before any launch (pointers never read)."""
    nat = pkg._native
    L = nat.lib()
    assert nat.EVAL_METRICS == 3
    header = open(os.path.join(REPO, "include", "gr_hip.h")).read()
    assert "#define GR_EVAL_METRICS 3" in header
    gv = pkg.torch_renderer.make_view(np.eye(4, dtype="float32"), np.eye(4, dtype="float32"), 50, 37, depth_grad=False)
    need = L.gr_eval_ws_bytes(ctypes.byref(gv))
    tiles = 4 * 3
    assert need >= 3 * 4 * tiles and need == 3 * L.gr_ssim_ws_bytes(37, 50, 3, 0)
    buf = (ctypes.c_float * 4)()
    p, null = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(0)
    assert L.gr_eval_view(ctypes.byref(gv), p, p, p, p, need - 1, null) == nat.GR_ERR_WORKSPACE
    assert b"workspace" in L.gr_last_error()
    for args in ((null, p, p, p), (p, null, p, p), (p, p, null, p), (p, p, p, null)):
        assert L.gr_eval_view(ctypes.byref(gv), *args, need, null) == nat.GR_ERR_INVALID_ARGUMENT
    for field, value in (("tile", 32), ("rows", 1)):
        bad = nat.GrView.from_buffer_copy(gv)
        setattr(bad, field, value)
        assert L.gr_eval_view(ctypes.byref(bad), p, p, p, p, need, null) == nat.GR_ERR_INVALID_ARGUMENT
    tall = nat.GrView.from_buffer_copy(gv)
    tall.width, tall.height = 1, 16 * 65535 + 1  # more tile rows than gr_ssim_fwd's grid takes
    assert L.gr_eval_ws_bytes(ctypes.byref(tall)) == 0
    assert L.gr_eval_view(ctypes.byref(tall), p, p, p, p, need, null) == nat.GR_ERR_INVALID_ARGUMENT
    cfg = nat.GrFitConfig(1, 1, 1, 1, 0, 0)  # (reduce_batch / reduce_tail are ignored)
    assert L.gr_eval_views(null, ctypes.byref(cfg), 1, None, 10, p, p, p, 3, p, p, null) == nat.GR_ERR_INVALID_ARGUMENT
    caps = (nat.GrPlan * 1)()
    cfg.caps = caps
    tgt = (nat.GrFitTarget * 1)()
    assert L.gr_eval_views(p, ctypes.byref(cfg), 1, tgt, 10, p, p, p, 3, p, p, null) == nat.GR_ERR_INVALID_ARGUMENT
    assert b"caps" in L.gr_last_error()
    cfg.caps = None
    assert L.gr_eval_views(p, ctypes.byref(cfg), 0, None, 10, p, p, p, 3, p, p, null) == nat.GR_OK  # no views: no-op
    assert L.gr_eval_views(p, ctypes.byref(cfg), 1, tgt, 0, p, p, p, 3, p, p, null) == nat.GR_OK  # no Gaussians: no-op
    assert callable(pkg.torch_renderer.eval_view_native)


def _golden_targets(fm, count=3):
    paths = sorted(os.path.join(GOLDEN, "fit_targets", f) for f in os.listdir(os.path.join(GOLDEN, "fit_targets"))
                   if f.endswith(".png"))[:count]
    assert len(paths) == count
    return [torch.from_numpy(fm._load_image(p, W, H)) for p in paths]


def _fitter(fm, **kw):
    torch.manual_seed(5)
    dev = torch.device("cpu")
    params = fm.build_params(N, dev, use_sh=False)
    with torch.no_grad():
        params["scales_raw"].fill_(-1.0)
        params["colors_raw"].add_(1.0)
    targets = _golden_targets(fm)
    cams = fm.orbit_cameras(len(targets), W, H, dev)
    return fm.ViewShardedFitter(params, cams, targets, W, H, **kw), cams, targets


def _dict_equal(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_evaluate_on_host_tensors(pkg, fm):
    fit, cams, targets = _fitter(fm)
    fit.step()
    got = fit.evaluate()
    assert sorted(got) == ["l1", "mean_l1", "mean_mse", "mean_psnr", "mean_ssim", "mse", "psnr", "ssim"]
    p = fit.canonical_params()
    with torch.no_grad():
        m, s, c, o = fm.activations(fit.params)
        for i, (cam, t) in enumerate(zip(cams, targets)):
            img = pkg.cpu_renderer.render(m, s, c, o, cam.view, cam.proj, W, H, torch.zeros(3))[0]
            want = pkg.losses.image_metrics(img, t)
            for k in ("l1", "mse", "ssim"):
                assert got[k][i] == float(want[k]), (k, i)
                assert got[k].dtype == np.float64
            assert got["psnr"][i] == -10.0 * np.log10(np.float64(float(want["mse"])))
    for k in ("l1", "mse", "psnr", "ssim"):
        assert got["mean_" + k] == float(got[k].mean()) and np.isfinite(got[k]).all()
    assert p["means"].shape[0] == N
    # held-out views passed explicitly, in the order passed
    sub = fit.evaluate([cams[2], cams[0]], [targets[2], targets[0]])
    for k in ("l1", "mse", "psnr", "ssim"):
        assert sub[k].tolist() == [got[k][2], got[k][0]]
    with pytest.raises(ValueError):
        fit.evaluate(cams, None)
    with pytest.raises(ValueError):
        fit.evaluate(cams[:2], targets)


def test_evaluate_does_not_change_the_fit(fm):
    a, _, _ = _fitter(fm, density_stats=True)
    b, _, _ = _fitter(fm, density_stats=True)
    la = [a.step() for _ in range(3)]
    lb = [b.step()]
    g0 = {k: v.grad.clone() for k, v in b.params.items()}
    rng = torch.get_rng_state()
    b.evaluate()
    assert torch.equal(rng, torch.get_rng_state())
    for k, v in b.params.items():
        assert torch.equal(v.grad, g0[k])
    lb += [b.step() for _ in range(2)]
    for x, y in zip(la, lb):
        assert torch.equal(x, y)
    for k in a.params:
        assert torch.equal(a.params[k], b.params[k]), k
    for x, y in zip(a.density_state(), b.density_state()):
        assert torch.equal(x, y)


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
    r = fit.evaluate()
    out_q.put((rank, len(fit.my_views), {k: np.asarray(v).copy() for k, v in r.items()}))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_gloo_ranks_return_the_single_process_dict(fm):
    fit, _, _ = _fitter(fm)
    want = fit.evaluate()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {r: (nv, d) for r, nv, d in (q.get(timeout=240) for _ in procs)}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert [res[r][0] for r in (0, 1)] == [2, 1]  # view i belongs to rank i % 2
    _dict_equal(res[0][1], res[1][1])
    _dict_equal(res[0][1], want)


def _main_args(tmp_path, *extra):
    return ["--targets_dir", os.path.join(GOLDEN, "fit_targets"), "--out_dir", str(tmp_path), "--iters", "4", "--width", str(W),
            "--height", str(H), "--num_gaussians", str(N), "--seed", "1", "--device", "cpu", *extra]


def test_cli_holdout(fm, tmp_path, monkeypatch, capsys):
    made = []

    class Spy(fm.ViewShardedFitter):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    monkeypatch.setattr(fm, "ViewShardedFitter", Spy)
    n_all = len([f for f in os.listdir(os.path.join(GOLDEN, "fit_targets")) if f.endswith(".png")])
    assert n_all == 3
    fm.main(_main_args(tmp_path, "--holdout_every", "3", "--eval_interval", "2"))
    log = json.loads((tmp_path / "eval.json").read_text())
    assert [e["iter"] for e in log] == [2, 4]
    assert len(made) == 1 and len(made[0].targets) == 2 and len(made[0].cams) == 2 and len(made[0].masks) == 2
    for e in log:
        assert e["views"] == [0] and e["n"] == N
        assert sorted(e) == ["iter", "l1", "mean_l1", "mean_psnr", "mean_ssim", "n", "psnr", "ssim", "views"]
        for k in ("psnr", "ssim", "l1"):
            assert len(e[k]) == 1 and math.isfinite(e[k][0]) and e["mean_" + k] == e[k][0]
    out = capsys.readouterr().out
    assert out.count("eval iter") == 2 and "held-out" in out


def test_cli_holdout_of_every_view_raises(fm, tmp_path):
    with pytest.raises(ValueError, match="no training view"):
        fm.main(_main_args(tmp_path, "--holdout_every", "1"))


def test_cli_evaluation_leaves_the_outputs_unchanged(fm, tmp_path):
    plain, evald = tmp_path / "plain", tmp_path / "eval"
    fm.main(_main_args(plain))
    fm.main(_main_args(evald, "--eval_interval", "2"))
    assert not (plain / "eval.json").exists()
    log = json.loads((evald / "eval.json").read_text())
    assert [e["iter"] for e in log] == [2, 4] and log[0]["views"] == [0, 1, 2]  # no hold-out: the training views
    for name in ("gaussians_fitted.npz", "loss.txt", "preview_view0.png"):
        assert (plain / name).read_bytes() == (evald / name).read_bytes(), name
