"""GPU: the parameter update's entries against one another, bit for bit.  gr_fit_param_steps (every parameter tensor's
gradient and Adam update in one launch) gives exactly what one gr_fit_param_step per tensor gives, for each activation and
with one to three stream accumulators, on both of its paths (float4 when the count is a multiple of 4 and every array
16-byte aligned, scalar otherwise); the gradient alone followed by gr_adam_step gives what the fused update gives; the
float4 and the scalar path agree; and a fit with more stream accumulators than one step sums folds the surplus."""
from __future__ import annotations

import ctypes
import importlib

import pytest
import torch


@pytest.mark.gpu
def test_param_steps_equal_per_tensor_steps(pkg, cuda):
    nat = pkg._native
    L = nat.lib()
    # (count, activation, accumulators, regulariser, element offset of every array): identity / softplus / sigmoid,
    # sizes across block boundaries; offset 1 misaligns a count that is a multiple of 4 (the scalar path)
    specs = [(3 * 1000, 0, 3, 0.0, 0), (3 * 777, 1, 2, 1e-4, 0), (1_000_003, 2, 1, 2e-6, 0), (255, 2, 0, 0.0, 0),
             (4_000_000, 1, 3, 1e-5, 0), (4096, 2, 2, 0.0, 1), (48 * 50_000, 0, 1, 0.0, 0)]
    b1, b2, eps = 0.9, 0.999, 1e-15
    runs = []
    for fused in (False, True):
        state = []
        for q, (n, act, na, reg, off) in enumerate(specs):
            gg = torch.Generator(device=cuda).manual_seed(10 + q)
            p = (torch.randn(n + off, generator=gg, device=cuda) * 3.0)[off:]
            m = (torch.randn(n + off, generator=gg, device=cuda) * 1e-3)[off:]
            v = (torch.rand(n + off, generator=gg, device=cuda) * 1e-6)[off:]
            accs = [torch.randn(n + off, generator=gg, device=cuda)[off:] for _ in range(na)]
            state.append((p, torch.empty(n + off, device=cuda)[off:], accs, m, v, act, reg, -(1e-3 / (1 - b1 ** (q + 2))),
                          (1 - b2 ** (q + 2)) ** 0.5))
        stream = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
        if fused:
            arr = (nat.GrParamStep * len(state))()
            for e, (p, gr, accs, m, v, act, reg, ns, bc) in zip(arr, state):
                e.count, e.act, e.num_accs = p.numel(), act, len(accs)
                e.param, e.grad = p.data_ptr(), gr.data_ptr()
                for j, x in enumerate(accs):
                    e.accs[j] = x.data_ptr()
                e.exp_avg, e.exp_avg_sq = m.data_ptr(), v.data_ptr()
                e.reg, e.neg_step_size, e.bias_correction2_sqrt = reg, ns, bc
            nat.check(L.gr_fit_param_steps(len(state), arr, ctypes.c_double(b1), ctypes.c_double(b2), ctypes.c_float(eps),
                                           stream), "gr_fit_param_steps")
        else:
            for p, gr, accs, m, v, act, reg, ns, bc in state:
                ptrs = (ctypes.c_void_p * max(1, len(accs)))(*[x.data_ptr() for x in accs])
                nat.check(L.gr_fit_param_step(p.numel(), act, nat.ptr(p), nat.ptr(gr), ptrs, len(accs), ctypes.c_float(reg),
                                              1, nat.ptr(m), nat.ptr(v), ctypes.c_float(ns), ctypes.c_float(bc),
                                              ctypes.c_double(b1), ctypes.c_double(b2), ctypes.c_float(eps), stream),
                          "gr_fit_param_step")
        torch.cuda.synchronize()
        runs.append([(p, gr, m, v) for p, gr, _, m, v, *_ in state])
    for a, b in zip(*runs):
        for x, y in zip(a, b):
            assert torch.equal(x, y)


@pytest.mark.gpu
@pytest.mark.parametrize("n,rgb", [(1, True), (1000, True), (300_001, False), (2_000_000, True)])
def test_fit_activations_match_torch(pkg, cuda, n, rgb):
    """gr_fit_activations (the fused step's activations, one launch) gives torch's softplus + 1e-3 and sigmoid bit for
    bit, across softplus's threshold (x > 20) and both tails of the sigmoid; its regulariser (reg_opacity * mean(o) +
    reg_scale * mean(s), the means in double) is torch's float32 value within 1e-6; the workspace counter is left
    zero (a second call, same results)."""
    fm = importlib.import_module("3dgaussian_amd.fit_multiview")
    gg = torch.Generator(device=cuda).manual_seed(n)
    params = {"means": torch.randn((n, 3), generator=gg, device=cuda),
              "scales_raw": torch.randn((n, 3), generator=gg, device=cuda) * 12.0,
              "opacities_raw": torch.randn((n,), generator=gg, device=cuda) * 40.0}
    if rgb:
        params["colors_raw"] = torch.randn((n, 3), generator=gg, device=cuda) * 30.0
    else:
        params["sh_raw"] = torch.randn((n, 16, 3), generator=gg, device=cuda)
    if n >= 4:  # the thresholds and tails exactly
        params["scales_raw"].view(-1)[:4] = torch.tensor([20.0, 20.000002, -104.0, 88.0], device=cuda)
        params["opacities_raw"][:4] = torch.tensor([-88.0, 104.0, 0.0, -1e-8], device=cuda)
    ws = torch.zeros(int(pkg._native.lib().gr_fit_activations_ws_bytes(n)), dtype=torch.uint8, device=cuda)
    w_o, w_s = 1e-3, 2.5e-4
    ref = fm.activations(params)
    ref_reg = float(w_o * ref[3].mean() + w_s * ref[1].mean())
    for _ in range(2):
        m, s, c, o, reg = fm.activations_native(params, (w_o, w_s), ws)
        torch.cuda.synchronize()
        assert m.data_ptr() == params["means"].data_ptr()
        assert torch.equal(s, ref[1]) and torch.equal(o, ref[3]) and torch.equal(c, ref[2])
        assert abs(float(reg) - ref_reg) <= 1e-6 * abs(ref_reg), (float(reg), ref_reg)
    _, s2, _, o2, none = fm.activations_native(params)  # no regulariser, no workspace
    assert none is None and torch.equal(s2, ref[1]) and torch.equal(o2, ref[3])


B1, B2, EPS = 0.9, 0.999, 1e-15
NEG_STEP, BC2S = -(1e-3 / (1 - B1 ** 3)), (1 - B2 ** 3) ** 0.5
PAD, CANARY = 4, 1234.5  # four floats each side keep a 16-byte alignment; the value no update produces


class _Arr:
    """count floats at element offset off of a canary-filled buffer."""

    def __init__(self, values, off=0):
        n = values.numel()
        self.buf = torch.full((PAD + off + n + PAD,), CANARY, device=values.device)
        self.t = self.buf[PAD + off:PAD + off + n]
        self.t.copy_(values)
        self.n, self.off = n, off

    def intact(self):
        return bool((self.buf[:PAD + self.off] == CANARY).all()) and bool((self.buf[PAD + self.off + self.n:] == CANARY).all())


def _data(n, act, na, cuda, seed):
    """(param, exp_avg, exp_avg_sq, accumulators): softplus inputs on both sides of its threshold 20.0 and sigmoid inputs
    at +-88 among the first elements."""
    gg = torch.Generator(device=cuda).manual_seed(seed)
    p = torch.randn(n, generator=gg, device=cuda) * 3.0
    edge = torch.tensor([20.0, 19.999998, 20.000002, 88.0, -88.0, 0.0, -20.0], device=cuda)
    if act == 2:
        edge = edge.flip(0)[2:]  # -88 first, so that a count of 1 or 3 sees it
    p[:min(n, edge.numel())] = edge[:n]
    m = torch.randn(n, generator=gg, device=cuda) * 1e-3
    v = torch.rand(n, generator=gg, device=cuda) * 1e-6
    return p, m, v, [torch.randn(n, generator=gg, device=cuda) for _ in range(na)]


def _stream(cuda):
    return ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)


def _param_step(nat, cuda, act, p, grad, accs, reg, adam, m, v):
    ptrs = (ctypes.c_void_p * max(1, len(accs)))(*[x.t.data_ptr() for x in accs])
    nat.check(nat.lib().gr_fit_param_step(p.n, act, nat.ptr(p.t), nat.ptr(grad.t if grad else None), ptrs, len(accs), reg, adam,
                                          nat.ptr(m.t if m else None), nat.ptr(v.t if v else None), NEG_STEP, BC2S, B1, B2, EPS,
                                          _stream(cuda)), "gr_fit_param_step")


def _entry(e, act, p, grad, accs, reg, m, v):
    e.count, e.act, e.num_accs = p.n, act, len(accs)
    e.param, e.grad, e.exp_avg, e.exp_avg_sq = p.t.data_ptr(), grad.t.data_ptr(), m.t.data_ptr(), v.t.data_ptr()
    for j, x in enumerate(accs):
        e.accs[j] = x.t.data_ptr()
    e.reg, e.neg_step_size, e.bias_correction2_sqrt = reg, NEG_STEP, BC2S


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 4, 255, 1028, 1_000_003])
def test_gradient_then_adam_equals_fused_step(pkg, cuda, n):
    """gr_fit_param_step(adam=0) then gr_adam_step on the stored gradient gives gr_fit_param_step(adam=1)'s param, exp_avg
    and exp_avg_sq bit for bit; adam=0 touches none of the three (with them, and with null moments) and nothing around any
    array; adam=1 without a gradient buffer gives the same three arrays."""
    nat = pkg._native
    L = nat.lib()
    reg = 1e-4
    for act in (nat.ACT_IDENTITY, nat.ACT_SOFTPLUS, nat.ACT_SIGMOID):
        for na in (0, 1, 3, 8):
            p0, m0, v0, a0 = _data(n, act, na, cuda, 100 * act + na)
            accs = [_Arr(x) for x in a0]

            def fresh():
                return _Arr(p0), _Arr(m0), _Arr(v0), _Arr(torch.full_like(p0, CANARY))

            p1, m1, v1, g1 = fresh()  # the fused update
            _param_step(nat, cuda, act, p1, g1, accs, reg, 1, m1, v1)
            p2, m2, v2, _ = fresh()  # the same without a gradient buffer
            _param_step(nat, cuda, act, p2, None, accs, reg, 1, m2, v2)
            p3, m3, v3, g3 = fresh()  # the gradient alone ...
            _param_step(nat, cuda, act, p3, g3, accs, reg, 0, m3, v3)
            g4 = _Arr(torch.full_like(p0, CANARY))  # ... and with null moments
            _param_step(nat, cuda, act, p3, g4, accs, reg, 0, None, None)
            torch.cuda.synchronize()
            what = (n, act, na)
            assert torch.equal(p3.t, p0) and torch.equal(m3.t, m0) and torch.equal(v3.t, v0), what
            assert torch.equal(g3.t, g1.t) and torch.equal(g4.t, g1.t), what
            assert bool(torch.isfinite(g1.t).all()) and not bool((g1.t == CANARY).any()), what
            nat.check(L.gr_adam_step(n, nat.ptr(p3.t), nat.ptr(g3.t), nat.ptr(m3.t), nat.ptr(v3.t), NEG_STEP, BC2S, B1, B2, EPS,
                                     _stream(cuda)), "gr_adam_step")
            torch.cuda.synchronize()
            for x, y in ((p1, p3), (m1, m3), (v1, v3), (p1, p2), (m1, m2), (v1, v2)):
                assert torch.equal(x.t, y.t), what
            assert not torch.equal(p1.t, p0), what
            for arr in (p1, m1, v1, g1, p2, m2, v2, p3, m3, v3, g3, g4, *accs):
                assert arr.intact(), what


def _both_entries(nat, cuda, specs, off, zero_between=False):
    """[(param, grad, exp_avg, exp_avg_sq)] of the specs' tensors, every array at element offset off, through one
    gr_fit_param_step per tensor and through one gr_fit_param_steps launch."""
    out = []
    for batched in (False, True):
        state = []
        for q, (n, act, na, reg) in enumerate(specs):
            p0, m0, v0, a0 = _data(n, act, na, cuda, 7 + q)
            state.append((act, _Arr(p0, off), _Arr(torch.full_like(p0, CANARY), off), [_Arr(x, off) for x in a0], reg,
                          _Arr(m0, off), _Arr(v0, off)))
            del p0, m0, v0, a0
        if batched:
            order = list(range(len(state)))
            if zero_between:
                order.insert(1, None)  # a tensor of no elements between two others
            arr = (nat.GrParamStep * len(order))()
            idle = _Arr(torch.zeros(4, device=cuda))
            for e, q in zip(arr, order):
                if q is None:
                    e.count, e.act, e.num_accs = 0, 1, 1
                    e.param = e.grad = e.exp_avg = e.exp_avg_sq = e.accs[0] = idle.t.data_ptr()
                else:
                    _entry(e, *state[q])
            nat.check(nat.lib().gr_fit_param_steps(len(order), arr, B1, B2, EPS, _stream(cuda)), "gr_fit_param_steps")
            torch.cuda.synchronize()
            assert idle.intact() and not bool(idle.t.any())
        else:
            for act, p, g, accs, reg, m, v in state:
                _param_step(nat, cuda, act, p, g, accs, reg, 1, m, v)
            torch.cuda.synchronize()
        for act, p, g, accs, reg, m, v in state:
            assert all(x.intact() for x in (p, g, m, v, *accs))
        out.append([(p.t, g.t, m.t, v.t) for _, p, g, _, _, m, v in state])
    return out


# the smallest counts at which a path grid-strides (16384 blocks of 256 threads per tensor): float4 when aligned, and scalar
STRIDE4, STRIDE1 = 4 * 256 * 16384 + 4 * 257, 256 * 16384 + 257


@pytest.mark.gpu
@pytest.mark.parametrize("specs", [[(1028, 0, 3, 0.0), (4, 1, 1, 1e-4), (4096, 2, 2, 2e-6), (256 * 4 * 3, 1, 8, 0.0)],
                                   [(STRIDE4, 1, 2, 1e-5)], [(STRIDE1, 2, 1, 2e-6)]],
                         ids=["small", "float4-stride", "scalar-stride"])
def test_float4_path_equals_scalar_path(pkg, cuda, specs):
    """The same data at element offset 0 (16-byte aligned: float4 where count % 4 == 0) and at offset 1 (scalar) gives equal
    bits, through the per-tensor and through the batched entry."""
    nat = pkg._native
    runs = _both_entries(nat, cuda, specs, 0) + _both_entries(nat, cuda, specs, 1)
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            for x, y in zip(a, b):
                assert torch.equal(x, y)


@pytest.mark.gpu
def test_batched_launch_skips_an_empty_tensor(pkg, cuda):
    """A count == 0 entry between two others: the two are updated as on their own, the empty one's arrays are untouched."""
    per_tensor, batched = _both_entries(pkg._native, cuda, [(1028, 1, 2, 1e-4), (255, 2, 3, 0.0)], 0, zero_between=True)
    for a, b in zip(per_tensor, batched):
        for x, y in zip(a, b):
            assert torch.equal(x, y)


@pytest.mark.gpu
def test_more_stream_accumulators_than_one_step_sums(pkg, cuda):
    """Nine streams over nine views leave nine accumulators per tensor, one more than a parameter step sums
    (FIT_MAX_ACC): the eager one-launch step folds the surplus and agrees with torch's autograd + Adam within
    test_fused_param_step_matches_torch_adam's tolerances."""
    import numpy as np

    fm = importlib.import_module("3dgaussian_amd.fit_multiview")
    bench = importlib.import_module("bench")
    W = H = 32
    assert 9 > pkg._native.FIT_MAX_ACC
    cams = fm.orbit_cameras(9, W, H, cuda)
    g = torch.Generator(device=cuda).manual_seed(9)
    targets = [torch.rand((H, W, 3), generator=g, device=cuda) for _ in cams]
    masks = [(t.mean(dim=2) > 0.5).float() for t in targets]
    saved = (fm.NUM_STREAMS, fm.GRAPH_MODE, fm.NATIVE_EXEC, fm.FUSED_STEP)
    fm.NUM_STREAMS, fm.GRAPH_MODE, fm.NATIVE_EXEC = 9, "0", "0"
    try:
        runs = []
        for fused in (False, True):
            fm.FUSED_STEP = fused
            f = fm.ViewShardedFitter(bench.synthetic_params(64, cuda), cams, targets, W, H, masks=masks)
            runs.append((float(f.step()), {k: v.detach().clone() for k, v in f.params.items()}))
    finally:
        fm.NUM_STREAMS, fm.GRAPH_MODE, fm.NATIVE_EXEC, fm.FUSED_STEP = saved
    (la, pa), (lf, pf) = runs
    np.testing.assert_allclose(lf, la, rtol=2e-6)
    for k in pa:
        err = float((pf[k] - pa[k]).norm() / pa[k].norm())
        assert err <= 1e-6, (k, err)
