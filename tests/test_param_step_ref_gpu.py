"""GPU: every element of the parameter update against a float64 reference (tests/param_step_reference.py).

tests/test_param_step_gpu.py compares the update's entries with one another, and a defect in act_backward / adam_elem
changes every side of those comparisons equally.  Here each entry (gr_fit_param_step with and without Adam,
gr_fit_param_steps, gr_adam_step) is held, element by element, to the bars of the reference's two stages: the gradient
from (x, accumulators, reg), then m', v' from the gradient the library wrote and p' from the library's own m', v'; on
data with the activations' thresholds and tails, cancelling accumulators, g g underflow, v = 0 against eps = 1e-15,
g ~ m, and t up to 100000.  Every pass of the three grid-stride loops is run and compared, bit for bit, with small calls
on the same elements, and gr_fit_param_steps_sched is called directly: the table row, the skip on overflow, the counter
and the flags.  The worst error / bar ratio of each test is printed (BARS lines; profiles/param_step_bars.txt)."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest
import torch

import param_step_reference as ps

PAD, CANARY = 4, 1234.5  # four floats each side keep a 16-byte alignment; the value no update produces
COUNTS = (1, 3, 4, 5, 255, 257, 1028)
NA = (0, 1, 2, 8)
TS = (1, 2, 1000, 100000)
ACTS = (ps.IDENTITY, ps.SOFTPLUS, ps.SIGMOID)


class _Arr:
    """count floats at element offset off of a canary-filled buffer."""

    def __init__(self, values, cuda, off=0):
        n = values if isinstance(values, int) else int(values.size if isinstance(values, np.ndarray) else values.numel())
        self.buf = torch.full((PAD + off + n + PAD,), CANARY, device=cuda)
        self.t = self.buf[PAD + off:PAD + off + n]
        if not isinstance(values, int):  # (a count alone: all canary)
            self.t.copy_(torch.as_tensor(values))
        self.n, self.off = n, off

    def intact(self):
        return bool((self.buf[:PAD + self.off] == CANARY).all()) and bool((self.buf[PAD + self.off + self.n:] == CANARY).all())

    def np(self):
        return self.t.cpu().numpy()


def _canary(n, cuda, off=0):
    return _Arr(int(n), cuda, off)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _stream(cuda):
    return ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)


@functools.lru_cache(maxsize=None)
def _data(act, na, t):
    return ps.data(2048, act, na, t)


@functools.lru_cache(maxsize=None)
def _adam_data(t):
    return ps.adam_data(2048, t)


def _head(d, n):
    x, m, v, accs = d
    return x[:n], m[:n], v[:n], [a[:n] for a in accs]


def _param_step(nat, cuda, act, p, grad, accs, reg, adam, m, v, sc):
    ptrs = (ctypes.c_void_p * max(1, len(accs)))(*[a.t.data_ptr() for a in accs])
    nat.check(nat.lib().gr_fit_param_step(p.n, act, nat.ptr(p.t), nat.ptr(grad.t), ptrs, len(accs), reg, adam, nat.ptr(m.t),
                                          nat.ptr(v.t), sc["ns"], sc["bc"], ps.B1, ps.B2, ps.EPS, _stream(cuda)),
              "gr_fit_param_step")


def _adam_step(nat, cuda, p, g, m, v, sc):
    nat.check(nat.lib().gr_adam_step(p.n, nat.ptr(p.t), nat.ptr(g.t), nat.ptr(m.t), nat.ptr(v.t), sc["ns"], sc["bc"], ps.B1,
                                     ps.B2, ps.EPS, _stream(cuda)), "gr_adam_step")


def _entry(e, act, p, grad, accs, reg, m, v, sc):
    e.count, e.act, e.num_accs = p.n, act, len(accs)
    e.param, e.grad, e.exp_avg, e.exp_avg_sq = p.t.data_ptr(), grad.t.data_ptr(), m.t.data_ptr(), v.t.data_ptr()
    for j, a in enumerate(accs):
        e.accs[j] = a.t.data_ptr()
    e.reg, e.neg_step_size, e.bias_correction2_sqrt = reg, sc["ns"], sc["bc"]


def _merge(worst, r):
    for k, x in r.items():
        worst[k] = max(worst.get(k, 0.0), x)


def _report(entry, what, worst):
    print("BARS", entry, what, " ".join(f"{k}={worst[k]:.3f}" for k in "gmvp" if k in worst))


class _Tensor:
    """One parameter tensor's operands on the device, every array canary-padded at element offset off."""

    def __init__(self, cuda, act, d, off):
        self.act, self.host = act, d
        x, m, v, accs = d
        self.p, self.m, self.v = _Arr(x, cuda, off), _Arr(m, cuda, off), _Arr(v, cuda, off)
        self.g = _canary(x.size, cuda, off)
        self.accs = [_Arr(a, cuda, off) for a in accs]

    def arrays(self):
        return (self.p, self.m, self.v, self.g, *self.accs)

    def check(self, sc, what, worst, adam=True):
        """After the update: nothing around any array changed, the accumulators unchanged, every output in its bar
        (adam: else p, m, v bit for bit as they were)."""
        x, m, v, accs = self.host
        assert all(a.intact() for a in self.arrays()), what
        assert all(_same_bits(a.np(), h) for a, h in zip(self.accs, accs)), what
        g32 = self.g.np()
        _merge(worst, ps.check_gradient(self.act, x, accs, ps.REG[self.act], g32, what))
        if adam:
            _merge(worst, ps.check_adam(g32, x, m, v, sc, self.p.np(), self.m.np(), self.v.np(), what))
        else:
            assert _same_bits(self.p.np(), x) and _same_bits(self.m.np(), m) and _same_bits(self.v.np(), v), what


@pytest.mark.gpu
@pytest.mark.parametrize("t", TS)
@pytest.mark.parametrize("act", ACTS, ids=ps.ACT_NAMES)
def test_param_step_elements_within_bars(pkg, cuda, act, t):
    """gr_fit_param_step with Adam (both stages) and without (the gradient; p, m, v untouched), every count, accumulator
    number and alignment: offset 0 takes the float4 path at counts 4 and 1028, offset 1 the scalar path."""
    nat = pkg._native
    sc = ps.scalars(t)
    for adam in (1, 0):
        worst = {}
        for n in COUNTS:
            for na in NA:
                for off in (0, 1):
                    T = _Tensor(cuda, act, _head(_data(act, na, t), n), off)
                    _param_step(nat, cuda, act, T.p, T.g, T.accs, ps.REG[act], adam, T.m, T.v, sc)
                    torch.cuda.synchronize()
                    T.check(sc, f"gr_fit_param_step adam={adam} {ps.ACT_NAMES[act]} n={n} na={na} off={off} t={t}", worst,
                            bool(adam))
        _report(f"gr_fit_param_step(adam={adam})", f"{ps.ACT_NAMES[act]} t={t}", worst)


BATCHES = [[(1028, ps.IDENTITY, 8), (5, ps.SOFTPLUS, 1), (257, ps.SIGMOID, 2), (255, ps.SOFTPLUS, 0)],
           [(4, ps.SIGMOID, 8), (1028, ps.SOFTPLUS, 2), (3, ps.IDENTITY, 1), (1, ps.SIGMOID, 0)]]


@pytest.mark.gpu
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("t", TS)
def test_param_steps_elements_within_bars(pkg, cuda, t, off):
    """gr_fit_param_steps: four tensors of different counts, activations and accumulator numbers in one launch, each
    entry with the scalars of its own step (t, the next of TS, ...)."""
    nat = pkg._native
    worst = {a: {} for a in ACTS}
    for specs in BATCHES:
        ts = [TS[(TS.index(t) + q) % len(TS)] for q in range(len(specs))]
        tensors = [_Tensor(cuda, act, _head(_data(act, na, tq), n), off) for (n, act, na), tq in zip(specs, ts)]
        arr = (nat.GrParamStep * len(tensors))()
        for e, T, tq in zip(arr, tensors, ts):
            _entry(e, T.act, T.p, T.g, T.accs, ps.REG[T.act], T.m, T.v, ps.scalars(tq))
        nat.check(nat.lib().gr_fit_param_steps(len(tensors), arr, ps.B1, ps.B2, ps.EPS, _stream(cuda)), "gr_fit_param_steps")
        torch.cuda.synchronize()
        for T, tq, (n, act, na) in zip(tensors, ts, specs):
            T.check(ps.scalars(tq), f"gr_fit_param_steps {ps.ACT_NAMES[act]} n={n} na={na} off={off} t={tq}", worst[act])
    for act in ACTS:
        _report("gr_fit_param_steps", f"{ps.ACT_NAMES[act]} t={t}.. off={off}", worst[act])


@pytest.mark.gpu
@pytest.mark.parametrize("t", TS)
def test_adam_step_elements_within_bars(pkg, cuda, t):
    """gr_adam_step on a gradient of magnitudes 1e-25 .. 1e17 with exact zeros and g ~ m."""
    nat = pkg._native
    sc = ps.scalars(t)
    worst = {}
    for n in COUNTS:
        for off in (0, 1):
            p0, g0, m0, v0 = (a[:n] for a in _adam_data(t))
            p, g, m, v = (_Arr(a, cuda, off) for a in (p0, g0, m0, v0))
            _adam_step(nat, cuda, p, g, m, v, sc)
            torch.cuda.synchronize()
            what = f"gr_adam_step n={n} off={off} t={t}"
            assert all(a.intact() for a in (p, g, m, v)) and _same_bits(g.np(), g0), what
            _merge(worst, ps.check_adam(g0, p0, m0, v0, sc, p.np(), m.np(), v.np(), what))
    _report("gr_adam_step", f"t={t}", worst)


# ---------------------------------------------------------------------------------------------------------------------
# Every pass of every grid-stride loop
# ---------------------------------------------------------------------------------------------------------------------
def _device_data(n, act, na, cuda, adam_only, starts):
    """The kind of data ps.data / ps.adam_data build, made on the device (16M elements), with the activation's edges
    at the head of every slice in ``starts``: (x, m, v, accs) or (p, g, m, v), torch tensors."""
    gg = torch.Generator(device=cuda).manual_seed(1000 + n % 1000)

    def rnd(kind):
        return (torch.randn if kind == "n" else torch.rand)(n, generator=gg, device=cuda)

    def spread(lo, hi):
        return torch.pow(10.0, rnd("u") * (hi - lo) + lo) * torch.where(rnd("u") < 0.5, -1.0, 1.0)

    m, v = rnd("n") * 1e-3, rnd("u") * 1e-6
    v[2::5] = 0.0
    v[4::9] = 1e-40
    if adam_only:
        p, g = rnd("n") * 3.0, spread(-25.0, 17.0)
        g[3::11] = 0.0
        m[5::13] = g[5::13] * (1.0 + 2.0 ** -21)
        return p, g, m, v
    x = rnd("n") * 6.0
    edge = torch.tensor(ps._EDGES_SIGMOID if act == ps.SIGMOID else ps._EDGES, device=cuda)
    for s in starts:
        x[s:s + edge.numel()] = edge
    accs = [spread(-6.0, 2.0) for _ in range(na)]
    if na >= 2:
        accs[1][::7] = -(accs[0][::7] * (1.0 + 2.0 ** -20))
    return x, m, v, accs


def _slices(count, first_pass):
    """The first 2048; the 4096 straddling the end of the first pass (cut at the count); the last 2048 and a tail of 3,
    which no float4 path takes."""
    return [(0, 2048), (first_pass - 2048, min(first_pass + 2048, count)), (count - 2051, count)]


STRIDES = [("scalar", 256 * 16384 + 259, 256 * 16384, ps.SIGMOID, 1), ("float4", 4 * 256 * 16384 + 1028, 4 * 256 * 16384, ps.SOFTPLUS, 2),
           ("adam", 4096 * 256 + 257, 4096 * 256, None, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("path,count,first_pass,act,na", STRIDES, ids=[s[0] for s in STRIDES])
def test_every_grid_stride_pass(pkg, cuda, path, count, first_pass, act, na):
    """The full array, then the same elements as small calls of their own on three slices: equal bits there (an
    element's result depends on neither the count nor its position), the float64 bars on those slices, and over the
    whole array no gradient element left at the canary and every output finite."""
    nat = pkg._native
    t = 3
    sc = ps.scalars(t)
    adam_only = path == "adam"
    assert (count % 4 == 0) == (path == "float4") and count > first_pass
    slices = _slices(count, first_pass)
    d = _device_data(count, act, na, cuda, adam_only, [a for a, _ in slices])

    def run(lo, hi):
        """The entry on elements [lo, hi) in buffers of their own: (p', m', v', g) canary-padded, and the host inputs."""
        if adam_only:
            p, g, m, v = (_Arr(a[lo:hi], cuda) for a in d)
            _adam_step(nat, cuda, p, g, m, v, sc)
            held = (p, g, m, v)
        else:
            x, m0, v0, accs0 = d
            p, m, v, g = _Arr(x[lo:hi], cuda), _Arr(m0[lo:hi], cuda), _Arr(v0[lo:hi], cuda), _canary(hi - lo, cuda)
            accs = [_Arr(a[lo:hi], cuda) for a in accs0]
            _param_step(nat, cuda, act, p, g, accs, ps.REG[act], 1, m, v, sc)
            held = (p, g, m, v, *accs)
        torch.cuda.synchronize()
        assert all(a.intact() for a in held), (path, lo, hi)
        return p, m, v, g

    full = run(0, count)
    for a in full:
        assert bool(torch.isfinite(a.t).all()), path
    if not adam_only:
        assert not bool((full[3].t == CANARY).any()), path
    worst = {}
    for lo, hi in slices:
        part = run(lo, hi)
        for a, b in zip(full, part):
            assert torch.equal(a.t[lo:hi].view(torch.int32), b.t.view(torch.int32)), (path, lo, hi)
        p1, m1, v1, g32 = (a.np() for a in part)
        what = f"{path} stride [{lo}, {hi})"
        if adam_only:
            p0, _, m0, v0 = (a[lo:hi].cpu().numpy() for a in d)
        else:
            p0, m0, v0 = (a[lo:hi].cpu().numpy() for a in d[:3])
            accs = [a[lo:hi].cpu().numpy() for a in d[3]]
            _merge(worst, ps.check_gradient(act, p0, accs, ps.REG[act], g32, what))
        _merge(worst, ps.check_adam(g32, p0, m0, v0, sc, p1, m1, v1, what))
    _report("gr_adam_step" if adam_only else "gr_fit_param_step(adam=1)", f"{path} stride count={count}", worst)


# ---------------------------------------------------------------------------------------------------------------------
# gr_fit_param_steps_sched, called directly
# ---------------------------------------------------------------------------------------------------------------------
SCHED_TS = (1, 2, 3, 5, 8, 13, 21, 34)  # row r of the table: update SCHED_TS[r]'s scalars, pairwise distinct in float32
SCHED_SPECS = [(1028, ps.SOFTPLUS, 2), (257, ps.SIGMOID, 1)]


class _Sched:
    def __init__(self, cuda, step, overflow):
        rows = [ps.scalars(t) for t in SCHED_TS]
        assert len({r["ns"] for r in rows}) == len(rows) and len({r["bc"] for r in rows}) == len(rows)
        self.rows = rows
        self.table = torch.tensor([[r["ns"], r["bc"]] for r in rows], dtype=torch.float32, device=cuda).reshape(-1)
        self.flags = torch.zeros(2, dtype=torch.int32, pin_memory=True)
        self.step = torch.tensor([step], dtype=torch.int32, device=cuda)
        self.ovf = torch.tensor([overflow], dtype=torch.int32, device=cuda)
        self.cuda = cuda

    def call(self, nat, tensors):
        """One gr_fit_param_steps_sched on the tensors; their entries carry scalars the schedule must replace."""
        assert 0 <= int(self.step) < len(self.rows)  # (never past the table)
        arr = (nat.GrParamStep * max(1, len(tensors)))()
        for e, T in zip(arr, tensors):
            _entry(e, T.act, T.p, T.g, T.accs, ps.REG[T.act], T.m, T.v, {"ns": -7.0, "bc": 0.25})
        nat.check(nat.lib().gr_fit_param_steps_sched(len(tensors), arr if tensors else None, ps.B1, ps.B2, ps.EPS,
                                                     nat.ptr(self.table), nat.ptr(self.step), nat.ptr(self.ovf),
                                                     ctypes.c_void_p(self.flags.data_ptr()), _stream(self.cuda)),
                  "gr_fit_param_steps_sched")
        torch.cuda.synchronize()

    def state(self):
        return int(self.step), int(self.ovf), self.flags.tolist()


def _sched_tensors(cuda):
    return [_Tensor(cuda, act, _head(_data(act, na, 2), n), 0) for n, act, na in SCHED_SPECS]


def _plain_steps(nat, cuda, sc):
    """gr_fit_param_steps on fresh copies of the same tensors with sc in the entries."""
    tensors = _sched_tensors(cuda)
    arr = (nat.GrParamStep * len(tensors))()
    for e, T in zip(arr, tensors):
        _entry(e, T.act, T.p, T.g, T.accs, ps.REG[T.act], T.m, T.v, sc)
    nat.check(nat.lib().gr_fit_param_steps(len(tensors), arr, ps.B1, ps.B2, ps.EPS, _stream(cuda)), "gr_fit_param_steps")
    torch.cuda.synchronize()
    return tensors


def _equal_tensors(a, b):
    return all(torch.equal(x.buf.view(torch.int32), y.buf.view(torch.int32))
               for S, T in zip(a, b) for x, y in zip(S.arrays(), T.arrays()))


@pytest.mark.gpu
@pytest.mark.parametrize("row", [0, 5, 7])
def test_sched_step_reads_its_row(pkg, cuda, row):
    """*step_dev = row, no overflow: the bits of gr_fit_param_steps with that row's scalars in the entries (the
    neighbouring rows give other bits), within the bars; then step_dev = row + 1 = flags[1], flags[0] = overflow = 0."""
    nat = pkg._native
    s = _Sched(cuda, row, 0)
    tensors = _sched_tensors(cuda)
    s.call(nat, tensors)
    assert _equal_tensors(tensors, _plain_steps(nat, cuda, s.rows[row]))
    for other in (row - 1, row + 1):
        if 0 <= other < len(s.rows):
            assert not _equal_tensors(tensors, _plain_steps(nat, cuda, s.rows[other])), other
    worst = {}
    for T in tensors:
        T.check(s.rows[row], f"gr_fit_param_steps_sched row {row}", worst)
    assert s.state() == (row + 1, 0, [0, row + 1])
    _report("gr_fit_param_steps_sched", f"row={row}", worst)


@pytest.mark.gpu
def test_sched_step_skips_on_overflow_and_the_flag_is_sticky(pkg, cuda):
    """*overflow = 1: p, m, v and the canary-filled gradient buffers untouched, the counter kept, flags = [1, t], the
    overflow cleared.  The next call, flags[0] not reset, updates as usual and leaves flags[0] = 1."""
    nat = pkg._native
    row = 5
    s = _Sched(cuda, row, 1)
    tensors, before = _sched_tensors(cuda), _sched_tensors(cuda)
    s.call(nat, tensors)
    assert _equal_tensors(tensors, before)
    assert all(bool((T.g.t == CANARY).all()) for T in tensors)
    assert s.state() == (row, 0, [1, row])
    s.call(nat, tensors)
    assert _equal_tensors(tensors, _plain_steps(nat, cuda, s.rows[row]))
    assert s.state() == (row + 1, 0, [1, row + 1])


@pytest.mark.gpu
def test_sched_step_without_tensors_advances_the_counter_only(pkg, cuda):
    nat = pkg._native
    s = _Sched(cuda, 3, 0)
    s.call(nat, [])
    assert s.state() == (4, 0, [0, 4])
    s.ovf.fill_(1)
    s.call(nat, [])
    assert s.state() == (4, 0, [1, 4])
