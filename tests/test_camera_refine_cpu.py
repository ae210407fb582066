"""CPU: camera pose refinement in the fit (fit_multiview.pose_view, ViewShardedFitter(refine_cameras=True), the CLI's
--refine_cameras) on host tensors, where the camera gradient comes from autograd through cpu_renderer, and the float64
helper tests/camera_reference.py against the F5 goldens (the reference's own autograd d view / d proj)."""
from __future__ import annotations

import importlib
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import GOLDEN, golden, golden_names
from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import camera_reference as cref  # noqa: E402

CAM_TOL = 1e-4  # tests/test_camera_grad.py's bar: relative L2 of d view / d proj
W, H, V, N = 64, 48, 4, 300


@pytest.fixture(scope="module")
def fm():
    return importlib.import_module("3dgaussian_amd.fit_multiview")


# ---- the recovery scene (shared with test_camera_refine_gpu.py) -------------------------------------------------------
def recovery_scene(fm, seed: int):
    """The scene of the recovery tests: (means, scales, colors, opacities) float32 arrays, the true cameras' (view,
    proj) float32 arrays, the perturbed initial views (float32) and the dense float64 targets at the true views."""
    rng = np.random.default_rng(seed)
    means = ((rng.random((N, 3)) - 0.5) * 1.2).astype(np.float32)
    scales = (rng.random((N, 3)) * 0.09 + 0.03).astype(np.float32)
    colors = (0.05 + 0.9 * rng.random((N, 3))).astype(np.float32)
    opac = (rng.random(N) * 0.5 + 0.3).astype(np.float32)
    cams = orc.orbit_cameras(V, W, H)
    init = []
    for i, (view, _) in enumerate(cams):
        a, t = rng.standard_normal(3), rng.standard_normal(3)
        p = np.concatenate([a / np.linalg.norm(a) * math.radians(2.0), t / np.linalg.norm(t) * 0.05])
        if i == 0:
            p[:] = 0.0
        v0 = fm.pose_view(torch.from_numpy(p), torch.from_numpy(np.asarray(view, np.float64)))
        init.append(v0.to(torch.float32).numpy())
    targets = [cref.render(means, scales, colors, opac, view, proj, W, H)[0].to(torch.float32) for view, proj in cams]
    return (means, scales, colors, opac), cams, init, targets


def exact_params(scene, device):
    """The fitter's raw parameters whose activations give the scene's own values (softplus + 1e-3, sigmoid)."""
    means, scales, colors, opac = (torch.from_numpy(a).double() for a in scene)
    inv_sig = lambda y: torch.log(y) - torch.log1p(-y)  # noqa: E731
    s = scales - 1e-3
    raw = {"means": means, "scales_raw": s + torch.log(-torch.expm1(-s)), "opacities_raw": inv_sig(opac),
           "colors_raw": inv_sig(colors)}
    return {k: torch.nn.Parameter(v.to(torch.float32).to(device)) for k, v in raw.items()}


def pose_errors(views, true_views):
    """Mean rotation error (radians) and mean camera-centre error over the views."""
    rot, cen = [], []
    for v, t in zip(views, true_views):
        v, t = np.asarray(v, np.float64), np.asarray(t, np.float64)
        c = (np.trace(v[:3, :3] @ t[:3, :3].T) - 1.0) / 2.0
        rot.append(math.acos(max(-1.0, min(1.0, c))))
        cen.append(float(np.linalg.norm(np.linalg.inv(v)[:3, 3] - np.linalg.inv(t)[:3, 3])))
    return float(np.mean(rot)), float(np.mean(cen))


def recovery_fitter(fm, seed: int, device, **kw):
    scene, cams, init, targets = recovery_scene(fm, seed)
    tr = importlib.import_module("3dgaussian_amd.torch_renderer")
    fc = [tr.Camera(view=torch.from_numpy(v).to(device), proj=torch.from_numpy(np.asarray(p, np.float32)).to(device))
          for v, (_, p) in zip(init, cams)]
    fit = fm.ViewShardedFitter(exact_params(scene, device), fc, [t.to(device) for t in targets], W, H, lr=0.0,
                               masks=None, reg_opacity=0.0, reg_scale=0.0, refine_cameras=True, camera_lr=2e-3,
                               camera_fixed=(0,), **kw)
    return fit, [np.asarray(v) for v, _ in cams], init


# ---- the helper against the goldens (passes on the parent) --------------------------------------------------------
@pytest.mark.parametrize("with_depth", [True, False])
@pytest.mark.parametrize("name", golden_names("f5_"))
def test_helper_matches_the_camera_goldens(name, with_depth):
    d = golden(name)
    dv, dp, *_ = cref.camera_grads(d["means"], d["scales"], d["colors"], d["opacities"], d["view"], d["proj"],
                                   int(d["width"]), int(d["height"]), d["g_rgb"], d["g_alpha"],
                                   d["g_depth"] if with_depth else None, background=d["background"])
    tag = "" if with_depth else "_nodepth"
    ev, ep = orc.rel_l2(dv.numpy(), d["d_view" + tag]), orc.rel_l2(dp.numpy(), d["d_proj" + tag])
    print(f"{name}{tag}: helper d_view relL2 {ev:.2e}, d_proj relL2 {ep:.2e}")
    assert ev <= CAM_TOL and ep <= CAM_TOL


# ---- pose_view --------------------------------------------------------------------------------------------------------
def test_pose_view(fm):
    V0 = torch.from_numpy(np.asarray(orc.orbit_cameras(4, W, H)[1][0], np.float64))
    for dt in (torch.float64, torch.float32):
        assert torch.equal(fm.pose_view(torch.zeros(6, dtype=torch.float64), V0.to(dt)), V0.to(dt))
    # the Jacobian at 0: the six generators applied to V0
    J = torch.autograd.functional.jacobian(lambda x: fm.pose_view(x, V0), torch.zeros(6, dtype=torch.float64))
    num = torch.stack([(fm.pose_view(torch.eye(6, dtype=torch.float64)[k] * 1e-6, V0)
                        - fm.pose_view(torch.eye(6, dtype=torch.float64)[k] * -1e-6, V0)) / 2e-6 for k in range(6)], dim=-1)
    gen = torch.zeros((6, 4, 4), dtype=torch.float64)
    gen[0, 2, 1], gen[0, 1, 2] = 1, -1
    gen[1, 0, 2], gen[1, 2, 0] = 1, -1
    gen[2, 1, 0], gen[2, 0, 1] = 1, -1
    for k in range(3):
        gen[3 + k, k, 3] = 1
    want = torch.stack([gen[k] @ V0 for k in range(6)], dim=-1)
    assert torch.allclose(J, want, rtol=0, atol=1e-14)
    assert torch.allclose(num, want, rtol=0, atol=1e-9)
    for mag in (1e-9, 1e-3, 1.0):
        w = torch.tensor([0.3, -0.5, 0.81], dtype=torch.float64)
        xi = torch.cat([w / w.norm() * mag, torch.tensor([0.1, 0.2, -0.3], dtype=torch.float64)])
        E = fm.pose_view(xi, torch.eye(4, dtype=torch.float64))
        R = E[:3, :3]
        assert torch.allclose(R @ R.T, torch.eye(3, dtype=torch.float64), rtol=0, atol=1e-15), mag
        assert abs(float(torch.linalg.det(R)) - 1.0) <= 1e-15
        assert torch.equal(E[:3, 3], xi[3:]) and torch.equal(E[3], torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64))
        assert torch.equal(fm.pose_view(xi, V0)[3], V0[3])
    # the rotation is the exponential: angle |omega| about omega
    xi = torch.tensor([0.0, 0.0, 0.5, 0, 0, 0], dtype=torch.float64)
    R = fm.pose_view(xi, torch.eye(4, dtype=torch.float64))[:3, :3]
    assert abs(float(R[0, 0]) - math.cos(0.5)) <= 1e-15 and abs(float(R[1, 0]) - math.sin(0.5)) <= 1e-15


# ---- the host fitter ----------------------------------------------------------------------------------------------
def _small_setup(fm, n=60):
    torch.manual_seed(7)
    dev = torch.device("cpu")
    params = fm.build_params(n, dev, use_sh=False)
    with torch.no_grad():
        params["scales_raw"].fill_(-1.5)
    cams = fm.orbit_cameras(V, W, H, dev)
    g = torch.Generator().manual_seed(3)
    targets = [torch.rand((H, W, 3), generator=g) for _ in range(V)]
    masks = [(t.mean(2) > 0.5).float() for t in targets]
    return params, cams, targets, masks


def test_host_fitter_gradient_is_autograd_through_pose_view(fm):
    """One step on the recovery scene: camera_state()'s gradient is torch.autograd.grad of the same loss through
    cpu_renderer and pose_view (the same code path: relative L2 <= 1e-6), the fixed row exactly zero."""
    tr = importlib.import_module("3dgaussian_amd.torch_renderer")
    fit, _, init = recovery_fitter(fm, 0, torch.device("cpu"))
    cams, targets = list(fit.cams), fit.targets
    fit.step()
    xi, g = fit.camera_state()
    assert xi.shape == (V, 6) and g.shape == (V, 6) and xi.dtype == torch.float64 and g.dtype == torch.float64
    assert not xi.is_cuda and not g.is_cuda
    m, s, c, o = fm.activations(fit.params)  # (lr = 0: the parameters of the step)
    xis = [torch.zeros(6, dtype=torch.float64, requires_grad=True) for _ in range(V)]
    total = 0.0
    for i in range(V):
        view = fm.pose_view(xis[i], cams[i].view.double()).to(torch.float32)
        pred, _, _ = tr.render_gaussians_torch(m, s, c, o, tr.Camera(view=view, proj=cams[i].proj), width=W, height=H,
                                               background=torch.zeros(3), max_gaussians=10000, return_aux=True,
                                               depth_grad=False)
        total = total + (pred - targets[i]).abs().mean()
    want = torch.stack(torch.autograd.grad(total / V, xis))
    assert torch.equal(g[0], torch.zeros(6, dtype=torch.float64)) and torch.equal(xi[0], torch.zeros(6, dtype=torch.float64))
    rel = float((g[1:] - want[1:]).norm() / want[1:].norm())
    print(f"host fitter d loss / d xi vs autograd by hand: relL2 {rel:.2e}")
    assert float(want[1:].norm()) > 0 and rel <= 1e-6
    # Adam's first step (its bias-corrected moments are g and g^2): camera_lr against the gradient; the cameras follow
    assert torch.allclose(xi[1:], -2e-3 * g[1:] / (g[1:].abs() + 1e-8), rtol=1e-9, atol=0)
    rc = fit.refined_cameras()
    assert torch.equal(rc[0].view, cams[0].view) and not torch.equal(rc[1].view, cams[1].view)
    assert torch.equal(rc[1].view, fm.pose_view(xi[1], cams[1].view.double()).float()) and rc[1].view is fit.cams[1].view
    assert torch.equal(rc[1].view[3], torch.tensor([0.0, 0.0, 0.0, 1.0]))


@pytest.mark.parametrize("seed", [0, 1])
def test_recovery(fm, seed):
    fit, true_views, init = recovery_fitter(fm, seed, torch.device("cpu"))
    r0, c0 = pose_errors(init, true_views)
    before = {k: v.detach().clone() for k, v in fit.params.items()}
    for _ in range(100):
        fit.step()
    r1, c1 = pose_errors([c.view.numpy() for c in fit.refined_cameras()], true_views)
    print(f"seed {seed}: rotation error {math.degrees(r0):.3f} -> {math.degrees(r1):.3f} deg (ratio {r1 / r0:.3f}), "
          f"centre error {c0:.4f} -> {c1:.4f} (ratio {c1 / c0:.3f})")
    assert all(torch.equal(before[k], fit.params[k].detach()) for k in before)  # lr = 0: the Gaussians stay exact
    assert r1 <= 0.25 * r0 and c1 <= 0.25 * c0


def test_off_is_off(fm):
    runs = []
    for kw in ({}, {"refine_cameras": False}):
        params, cams, targets, masks = _small_setup(fm)
        fit = fm.ViewShardedFitter(params, cams, targets, W, H, masks=masks, **kw)
        losses = [fit.step().clone() for _ in range(3)]
        runs.append((losses, {k: v.detach().clone() for k, v in fit.params.items()}, fit))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b)
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
    with pytest.raises(ValueError, match="refine_cameras"):
        runs[1][2].camera_state()
    assert runs[1][2].refine_cameras is False


def test_densify_leaves_the_pose_optimiser_alone(fm):
    params, cams, targets, masks = _small_setup(fm)
    fit = fm.ViewShardedFitter(params, cams, targets, W, H, masks=masks, refine_cameras=True)
    fit.step()
    opt, xi = fit._cam_opt, fit.camera_state()[0]
    fit.densify_and_prune(max_gaussians=80, densify_ratio=0.2, prune_opacity=0.05)
    fit.reset_optimizer()
    assert fit._cam_opt is opt and torch.equal(fit.camera_state()[0], xi) and len(opt.state) == 1
    fit.step()
    assert not torch.equal(fit.camera_state()[0], xi)


def test_bad_fixed_index_raises(fm):
    params, cams, targets, masks = _small_setup(fm)
    with pytest.raises(ValueError, match="camera_fixed"):
        fm.ViewShardedFitter(params, cams, targets, W, H, masks=masks, refine_cameras=True, camera_fixed=(V,))


# ---- two gloo ranks ---------------------------------------------------------------------------------------------------
def _worker(rank, world, port, out_q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, REPO)
    fm = importlib.import_module("3dgaussian_amd.fit_multiview")
    params, cams, targets, masks = _small_setup(fm)
    fit = fm.ViewShardedFitter(params, cams, targets, W, H, masks=masks, refine_cameras=True)
    for _ in range(3):
        fit.step()
    xi, g = fit.camera_state()
    out_q.put((rank, xi.numpy().copy(), g.numpy().copy(), np.stack([c.view.numpy() for c in fit.refined_cameras()])))
    dist.barrier()
    dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.timeout(300)
def test_two_gloo_ranks_keep_identical_cameras(fm):
    params, cams, targets, masks = _small_setup(fm)
    ref = fm.ViewShardedFitter(params, cams, targets, W, H, masks=masks, refine_cameras=True)
    for _ in range(3):
        ref.step()
    ref_xi, ref_g = ref.camera_state()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {r: (xi, g, views) for r, xi, g, views in (q.get(timeout=240) for _ in procs)}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for a, b in zip(res[0], res[1]):
        assert a.tobytes() == b.tobytes()  # bit-identical on both ranks
    assert np.abs(res[0][0]).max() > 0
    torch.testing.assert_close(torch.from_numpy(res[0][0]), ref_xi, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(torch.from_numpy(res[0][1]), ref_g, rtol=1e-5, atol=1e-6)


# ---- the CLI ----------------------------------------------------------------------------------------------------------
def _main_args(out, *extra):
    return ["--targets_dir", os.path.join(GOLDEN, "fit_targets"), "--out_dir", str(out), "--iters", "3", "--width", "32",
            "--height", "24", "--num_gaussians", "40", "--seed", "1", "--device", "cpu", *extra]


def test_cli_writes_the_refined_cameras(fm, tmp_path, capsys):
    plain, ref, held = tmp_path / "plain", tmp_path / "ref", tmp_path / "held"
    fm.main(_main_args(plain))
    assert not (plain / "cameras_refined.npz").exists()
    fm.main(_main_args(ref, "--refine_cameras", "--camera_lr", "2e-3"))
    with np.load(ref / "cameras_refined.npz") as d:
        view, proj = d["view"], d["proj"]
    want = fm.orbit_cameras(3, 32, 24, torch.device("cpu"))
    assert view.shape == (3, 4, 4) and proj.shape == (3, 4, 4) and view.dtype == np.float32 and proj.dtype == np.float32
    assert np.array_equal(view[0], want[0].view.numpy())  # --camera_fix 0 (the default)
    assert not np.array_equal(view[1], want[1].view.numpy()) and not np.array_equal(view[2], want[2].view.numpy())
    assert all(np.array_equal(proj[i], want[i].proj.numpy()) for i in range(3))
    # the file is the --camera_npz schema: it can be fed back; no fixed view: every pose moves
    fm.main(_main_args(tmp_path / "again", "--refine_cameras", "--camera_fix", "none", "--camera_npz",
                       str(ref / "cameras_refined.npz")))
    with np.load(tmp_path / "again" / "cameras_refined.npz") as d:
        assert d["view"].shape == (3, 4, 4) and not np.array_equal(d["view"][0], view[0])
    # held-out views keep their input poses, and a line says so
    capsys.readouterr()
    fm.main(_main_args(held, "--refine_cameras", "--holdout_every", "3", "--camera_fix", "none"))
    assert "held-out views keep their input poses" in capsys.readouterr().out
    with np.load(held / "cameras_refined.npz") as d:
        assert np.array_equal(d["view"][0], want[0].view.numpy()) and not np.array_equal(d["view"][1], want[1].view.numpy())
