"""CPU: the fused D-SSIM fit path's surface without a device: the new C entries in the header, the bindings and the
host-only library (argument checks before any launch), the dssim_fused switch of ViewShardedFitter and
fit_multiview.main on host tensors (where it has no effect)."""
from __future__ import annotations

import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO

ENTRIES = ("gr_bwd_ssim_bytes", "gr_bwd_fit_ssim", "gr_bwd_fit_ssim_gather", "gr_fit_views_ssim")


@pytest.fixture(scope="module")
def fm(pkg):
    return importlib.import_module("3dgaussian_amd.fit_multiview")


def test_header_and_bindings_declare_the_entries(pkg):
    nat = pkg._native
    header = open(os.path.join(REPO, "include", "gr_hip.h")).read()
    L = nat.lib()
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in nat._SIG and getattr(L, name).argtypes == nat._SIG[name][1]
    # each takes its older sibling's arguments plus one float (w_dssim)
    for new, old in (("gr_bwd_fit_ssim", "gr_bwd_fit"), ("gr_bwd_fit_ssim_gather", "gr_bwd_fit_gather"),
                     ("gr_fit_views_ssim", "gr_fit_views")):
        a, b = list(nat._SIG[new][1]), list(nat._SIG[old][1])
        assert len(a) == len(b) + 1
        del a[len(a) - 1 - a[::-1].index(ctypes.c_float)]  # (the last float: w_dssim follows g_scale)
        assert a == b
    tr = pkg.torch_renderer
    assert callable(tr.backward_fit_ssim_native) and callable(tr.backward_fit_ssim_gather_native)


def test_abi_sizes_and_argument_checks(pkg):
    """gr_bwd_ssim_bytes and the checks that come before any launch: the pointers here are never dereferenced."""
    nat = pkg._native
    L = nat.lib()
    gv = pkg.torch_renderer.make_view(np.eye(4, dtype="float32"), np.eye(4, dtype="float32"), 50, 37, depth_grad=False)
    plan = nat.GrPlan(100, 200, 100)
    need = L.gr_bwd_ssim_bytes(ctypes.byref(gv), 10, ctypes.byref(plan))
    assert need >= L.gr_bwd_bytes(ctypes.byref(gv), 10, ctypes.byref(plan)) + L.gr_ssim_ws_bytes(37, 50, 3, 1)
    buf = (ctypes.c_float * 4)()
    p, null = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(0)

    def gather(view, lam, ws_bytes, target=p):
        return L.gr_bwd_fit_ssim_gather(ctypes.byref(view), 10, ctypes.byref(plan), p, p, p, target, null, ctypes.c_float(0.2),
                                        null, ctypes.c_float(0.0), ctypes.c_float(1.0), ctypes.c_float(lam), p, p, ws_bytes,
                                        p, null, null)

    for lam in (1.5, -0.25, float("nan")):
        assert gather(gv, lam, need) == nat.GR_ERR_INVALID_ARGUMENT and b"w_dssim" in L.gr_last_error()
    assert gather(gv, 0.2, need, target=null) == nat.GR_ERR_INVALID_ARGUMENT
    assert gather(gv, 0.2, need - 1) == nat.GR_ERR_WORKSPACE and b"workspace" in L.gr_last_error()
    assert gather(gv, 0.0, need - 1) == nat.GR_ERR_WORKSPACE  # one workspace contract for every weight
    for field, value in (("tile", 32), ("rows", 1)):
        bad = nat.GrView.from_buffer_copy(gv)
        setattr(bad, field, value)
        assert gather(bad, 0.2, need) == nat.GR_ERR_INVALID_ARGUMENT
    full = L.gr_bwd_fit_ssim(ctypes.byref(gv), 10, ctypes.byref(plan), p, p, p, 3, p, p, p, p, p, null, ctypes.c_float(0.2),
                             null, ctypes.c_float(0.0), ctypes.c_float(1.0), ctypes.c_float(2.0), p, p, p, p, p, 0, p, need,
                             null)
    assert full == nat.GR_ERR_INVALID_ARGUMENT and b"w_dssim" in L.gr_last_error()
    cfg = nat.GrFitConfig(1, 1, 1, 1, 1, 0)
    st = L.gr_fit_views_ssim(p, ctypes.byref(cfg), 1, None, 10, p, p, p, 3, p, ctypes.c_float(0.2), ctypes.c_float(0.0),
                             ctypes.c_float(1.0), ctypes.c_float(1.5), p, None, null)
    assert st == nat.GR_ERR_INVALID_ARGUMENT and b"w_dssim" in L.gr_last_error()


def _scene(fm, n_views=2, n=40, W=24, H=20):
    torch.manual_seed(7)
    dev = torch.device("cpu")
    params = fm.build_params(n, dev, use_sh=False)
    with torch.no_grad():
        params["scales_raw"].fill_(-1.0)
    cams = fm.orbit_cameras(n_views, W, H, dev)
    g = torch.Generator().manual_seed(3)
    targets = [torch.rand((H, W, 3), generator=g) for _ in cams]
    return params, cams, targets, W, H


def _clone(params):
    return {k: torch.nn.Parameter(v.detach().clone()) for k, v in params.items()}


def test_flag_has_no_effect_on_host_tensors(fm):
    params, cams, targets, W, H = _scene(fm)
    masks = [(t.mean(2) > 0.5).float() for t in targets]
    a = fm.ViewShardedFitter(_clone(params), cams, targets, W, H, masks=masks, dssim_weight=0.2)
    b = fm.ViewShardedFitter(_clone(params), cams, targets, W, H, masks=masks, dssim_weight=0.2, dssim_fused=True)
    cpu = torch.device("cpu")
    assert not a._direct(cpu) and not b._direct(cpu) and not b._graph_ok(cpu) and not b._bands_ok()
    assert torch.equal(a.step(), b.step())
    for k in a.params:
        assert torch.equal(a.params[k].grad, b.params[k].grad), k
        assert torch.equal(a.params[k].detach(), b.params[k].detach()), k


def test_flag_without_a_dssim_term_changes_nothing(fm):
    """dssim_fused with l = 0: _direct() is what it is today on any device, and no D-SSIM form is selected."""
    params, cams, targets, W, H = _scene(fm)
    a = fm.ViewShardedFitter(_clone(params), cams, targets, W, H)
    b = fm.ViewShardedFitter(_clone(params), cams, targets, W, H, dssim_fused=True)
    assert a.dssim_fused is False and b.dssim_fused is True and not b._ssim_form()
    for dev in (torch.device("cpu"), torch.device("cuda:0")):  # (no device is touched: the answer depends on its type)
        assert a._direct(dev) == b._direct(dev)
    assert b._direct(torch.device("cuda:0")) == (fm.FUSED_LOSS and fm.DIRECT_BACKWARD)
    c = fm.ViewShardedFitter(_clone(params), cams, targets, W, H, dssim_weight=0.2, dssim_fused=True)
    assert c._ssim_form() and not c._bands_ok()
    # the switch follows the device: the fused form on the HIP device only, and never with a foreign render function
    assert c._direct(torch.device("cuda:0")) == (fm.FUSED_LOSS and fm.DIRECT_BACKWARD) and not c._direct(torch.device("cpu"))
    d = fm.ViewShardedFitter(_clone(params), cams, targets, W, H, dssim_weight=0.2, dssim_fused=True,
                             render_fn=lambda *a, **kw: fm.hip_render(*a, **kw))
    assert not d._direct(torch.device("cuda:0"))
    assert torch.equal(a.step(), b.step())


def test_main_accepts_dssim_fused_on_cpu(fm, tmp_path):
    fm.main(["--targets_dir", os.path.join(GOLDEN, "fit_targets"), "--out_dir", str(tmp_path), "--iters", "2",
             "--width", "32", "--height", "32", "--num_gaussians", "60", "--seed", "1", "--device", "cpu",
             "--dssim_weight", "0.2", "--dssim_fused"])
    assert len((tmp_path / "loss.txt").read_text().split()) == 2
