"""CPU: the parameter update's element-wise bars (tests/param_step_reference.py) are neither vacuous nor unreachable.

* torch's own float32 CPU step (autograd through softplus(x) + 1e-3 / sigmoid / identity, then torch.optim.Adam with
  eps = 1e-15 at t = 1, 2, 1000) lies inside the bars against the float64 reference on the data of the GPU tests: the
  reference side alone passes;
* a float32 emulation of the kernel passes them too, and with one injected defect each it fails them, whatever the
  aggregate relative L2 of 1e-6 (test_fused_param_step_matches_torch_adam's check) says, which is printed;
* ViewShardedFitter._graph_sched's row t holds the float32 of the eager step's two expressions for update t + 1.
"""
from __future__ import annotations

import importlib
import types

import numpy as np
import pytest
import torch

import param_step_reference as ps

F = np.float32
NA = (0, 1, 2, 8)
N = 2048


def _torch_step(act, x, accs, reg, m, v, t):
    """torch, float32, CPU: (g, p', m', v') of one Adam step on the activation's backward of the summed accumulators."""
    p = torch.nn.Parameter(torch.from_numpy(x.copy()))
    s = torch.from_numpy(accs[0].copy()) if accs else torch.zeros_like(p)
    for a in accs[1:]:
        s = s + torch.from_numpy(a)
    s = s + torch.tensor(reg, dtype=torch.float32)
    y = (torch.nn.functional.softplus(p) + 1e-3) if act == ps.SOFTPLUS else torch.sigmoid(p) if act == ps.SIGMOID else p * 1.0
    y.backward(gradient=s)
    g = p.grad.detach().clone()
    opt = torch.optim.Adam([p], lr=ps.LR, betas=(ps.B1, ps.B2), eps=ps.EPS, foreach=False)
    opt.state[p] = {"step": torch.tensor(float(t - 1)), "exp_avg": torch.from_numpy(m.copy()),
                    "exp_avg_sq": torch.from_numpy(v.copy())}
    opt.step()
    st = opt.state[p]
    assert float(st["step"]) == t
    return g.numpy(), p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


@pytest.mark.parametrize("t", [1, 2, 1000])
@pytest.mark.parametrize("act", [ps.IDENTITY, ps.SOFTPLUS, ps.SIGMOID], ids=ps.ACT_NAMES)
def test_torch_cpu_step_is_inside_the_bars(act, t):
    sc = ps.scalars(t)
    for na in NA:
        x, m, v, accs = ps.data(N, act, na, t)
        g, p1, m1, v1 = _torch_step(act, x, accs, ps.REG[act], m, v, t)
        what = f"torch {ps.ACT_NAMES[act]} na={na} t={t}"
        r = ps.check_gradient(act, x, accs, ps.REG[act], g, what)
        r.update(ps.check_adam(g, x, m, v, sc, p1, m1, v1, what))
        print("BARS torch-cpu", ps.ACT_NAMES[act], f"na={na} t={t}", " ".join(f"{k}={r[k]:.3f}" for k in "gmvp"))


@pytest.mark.parametrize("t", [1, 2, 1000])
def test_torch_cpu_adam_is_inside_the_bars_on_the_direct_data(t):
    """gr_adam_step's data (|g| from 1e-25 to 1e17, zeros, g ~ m) through torch.optim.Adam alone."""
    p, g, m, v = ps.adam_data(N, t)
    q = torch.nn.Parameter(torch.from_numpy(p.copy()))
    q.grad = torch.from_numpy(g.copy())
    opt = torch.optim.Adam([q], lr=ps.LR, betas=(ps.B1, ps.B2), eps=ps.EPS, foreach=False)
    opt.state[q] = {"step": torch.tensor(float(t - 1)), "exp_avg": torch.from_numpy(m.copy()),
                    "exp_avg_sq": torch.from_numpy(v.copy())}
    opt.step()
    st = opt.state[q]
    r = ps.check_adam(g, p, m, v, ps.scalars(t), q.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy(),
                      f"torch adam t={t}")
    print("BARS torch-cpu adam", f"t={t}", " ".join(f"{k}={r[k]:.3f}" for k in "mvp"))


@pytest.mark.parametrize("t", [1, 2, 1000, 100000])
def test_emulated_kernel_is_inside_the_bars(t):
    sc = ps.scalars(t)
    for act in (ps.IDENTITY, ps.SOFTPLUS, ps.SIGMOID):
        for na in NA:
            x, m, v, accs = ps.data(N, act, na, t)
            g = ps.emulate_gradient(act, x, accs, ps.REG[act])
            p1, m1, v1 = ps.emulate_adam(g, x, m, v, sc)
            what = f"emulation {ps.ACT_NAMES[act]} na={na} t={t}"
            ps.check_gradient(act, x, accs, ps.REG[act], g, what)
            ps.check_adam(g, x, m, v, sc, p1, m1, v1, what)
    p, g, m, v = ps.adam_data(N, t)
    p1, m1, v1 = ps.emulate_adam(g, p, m, v, sc)
    ps.check_adam(g, p, m, v, sc, p1, m1, v1, f"emulation adam t={t}")


def _rel_l2(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# (defect, activation, accumulators, t, count)
DEFECT_CASES = [("softplus_threshold_2", ps.SOFTPLUS, 2, 2, N), ("first_pass_only", ps.IDENTITY, 1, 2, ps.FIRST_PASS + 257),
                ("bias_correction_of_t_minus_1", ps.SOFTPLUS, 2, 2, N), ("eps_inside_sqrt", ps.IDENTITY, 0, 2, N),
                ("eighth_accumulator_dropped", ps.IDENTITY, 8, 2, N), ("one_minus_y_is_1_above_15", ps.SIGMOID, 2, 2, N)]


@pytest.mark.parametrize("defect,act,na,t,n", DEFECT_CASES, ids=[c[0] for c in DEFECT_CASES])
def test_bars_reject_a_defect(defect, act, na, t, n):
    """The emulated kernel with one defect: some element of some output leaves its bar (the intact emulation of the same
    data stays inside).  Whether the parameters' relative L2 against the intact run stays within 1e-6 is printed."""
    assert defect in ps.DEFECTS
    x, m, v, accs = ps.data(n, act, na, t)
    reg = ps.REG[act]
    if defect == "eps_inside_sqrt":  # Adam alone, on the direct data (v = 0 and g g = 0 are where eps decides)
        x, g_in, m, v = ps.adam_data(n, t)
    sc = ps.scalars(t)
    outs = {}
    for d in (None, defect):
        g = g_in if defect == "eps_inside_sqrt" else ps.emulate_gradient(act, x, accs, reg, d)
        used = ps.scalars(t - 1) if d == "bias_correction_of_t_minus_1" else sc
        outs[d] = (g,) + ps.emulate_adam(g, x, m, v, used, d)

    def worst(out):
        g, p1, m1, v1 = out
        gr, gb, _ = ps.gradient(act, x, accs, reg)
        (mr, mb), (vr, vb) = ps.moments(g, m, v, sc)
        pr, pb = ps.param(x, m1, v1, sc)
        w = {"m": ps.ratios(m1, mr, mb).max(), "v": ps.ratios(v1, vr, vb).max(), "p": ps.ratios(p1, pr, pb).max()}
        if defect != "eps_inside_sqrt":
            w["g"] = ps.ratios(g, gr, gb).max()
        return w

    good, bad = worst(outs[None]), worst(outs[defect])
    assert max(good.values()) <= 1.0, good
    assert max(bad.values()) > 1.0, bad
    # the aggregate check, on data of the kind it runs on (benign_data), through the fused step with the same defect
    bx, bm, bv, baccs = ps.benign_data(n, max(na, 1))
    runs = []
    for d in (None, defect):
        g = ps.emulate_gradient(act, bx, baccs, reg, d)
        runs.append(ps.emulate_adam(g, bx, bm, bv, ps.scalars(t - 1) if d == "bias_correction_of_t_minus_1" else sc, d)[0])
    agg = _rel_l2(runs[1], runs[0])
    print(f"DEFECT {defect}: worst error/bar " + " ".join(f"{k}={bad[k]:.3g}" for k in sorted(bad)) +
          f"; rejected by the bars: yes; parameters' relative L2 on benign data {agg:.3e}, aggregate 1e-6 check "
          f"{'passes it' if agg <= 1e-6 else 'rejects it'}")


def _fitter_stub(lr, b1, b2):
    return types.SimpleNamespace(opt=types.SimpleNamespace(param_groups=[{"lr": lr, "betas": (b1, b2)}]))


@pytest.mark.parametrize("t0,rows", [(0, 1 << 16), (40000, 2 * 40001)])
def test_graph_sched_rows_are_the_eager_steps_scalars(pkg, t0, rows):
    """Row t is what the eager step hands the library for update t + 1 (_fused_param_step's two expressions through
    ctypes.c_float); beyond t0 = 32768 the table covers 2 (t0 + 1) rows."""
    fm = importlib.import_module("3dgaussian_amd.fit_multiview")
    lr, b1, b2 = 1.6e-4, 0.9, 0.999
    tab, T = fm.ViewShardedFitter._graph_sched(_fitter_stub(lr, b1, b2), torch.device("cpu"), t0)
    assert T == rows and tab.dtype == torch.float32 and tab.numel() == 2 * T
    tab = tab.numpy().reshape(T, 2)
    import ctypes

    for t in (0, 1, 999, 65535, T - 1):
        u = float(t + 1)  # the eager step: st["step"] += 1; t = float(st["step"])
        want = (ctypes.c_float(-(lr / (1.0 - b1 ** u))).value, ctypes.c_float((1.0 - b2 ** u) ** 0.5).value)
        assert (float(tab[t, 0]), float(tab[t, 1])) == want, t
    assert tab[0, 0] != tab[1, 0] and tab[0, 1] != tab[1, 1]  # (a row off by one would show)
    assert np.all(np.isfinite(tab)) and np.all(tab[:, 0] < 0) and np.all(tab[:, 1] > 0)
