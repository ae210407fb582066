"""CPU: the refusals of the parameter update's four entries (gr_fit_param_step, gr_fit_param_steps,
gr_fit_param_steps_sched, gr_adam_step), each with its status and the exact gr_last_error() text, and where two apply
the one that comes first.  Every one returns before any launch, as do the calls with nothing to do (count 0, no
entries), which return GR_OK.  The expected strings are written out here, never read from the library.  No pointer is
dereferenced."""
from __future__ import annotations

import ctypes

import pytest

OK, INVALID = 0, 1  # GR_OK, GR_ERR_INVALID_ARGUMENT
_BUF = (ctypes.c_float * 4)()
P = ctypes.cast(_BUF, ctypes.c_void_p).value  # a non-null pointer (never dereferenced)
NULL = None
B1, B2, EPS = 0.9, 0.999, 1e-15

STEP_BAD = "gr_fit_param_step: bad arguments"
STEP_ACC = "gr_fit_param_step: null accumulator"
STEPS_BAD = "gr_fit_param_steps: bad arguments"
STEPS_ENTRY = "gr_fit_param_steps: bad parameter entry"
STEPS_ACC = "gr_fit_param_steps: null accumulator"
SCHED_NULL = "gr_fit_param_steps_sched: null schedule, counter, overflow or flags"
SCHED_PINNED = "gr_fit_param_steps_sched: host_flags must be pinned host memory"
ADAM_BAD = "gr_adam_step: bad arguments"


def _accs(*ptrs):
    return (ctypes.c_void_p * max(1, len(ptrs)))(*ptrs)


def _step(L, **over):
    a = dict(count=10, act=1, param=P, grad=P, accs=_accs(P, P), num_accs=2, adam=1, exp_avg=P, exp_avg_sq=P)
    a.update(over)
    got = L.gr_fit_param_step(a["count"], a["act"], a["param"], a["grad"], a["accs"], a["num_accs"], 1e-4, a["adam"],
                              a["exp_avg"], a["exp_avg_sq"], -1e-3, 0.5, B1, B2, EPS, NULL)
    return got, L.gr_last_error().decode()


STEP = [
    ("count < 0", dict(count=-1), STEP_BAD),
    ("act < 0", dict(act=-1), STEP_BAD),
    ("act > 2", dict(act=3), STEP_BAD),
    ("null param", dict(param=NULL), STEP_BAD),
    ("adam, null exp_avg", dict(exp_avg=NULL), STEP_BAD),
    ("adam, null exp_avg_sq", dict(exp_avg_sq=NULL), STEP_BAD),
    ("no adam, null grad", dict(adam=0, grad=NULL), STEP_BAD),
    ("num_accs < 0", dict(num_accs=-1), STEP_BAD),
    ("num_accs > GR_FIT_MAX_ACC", dict(num_accs=9), STEP_BAD),
    ("accumulators without a list", dict(accs=NULL), STEP_BAD),
    ("count 0, null param", dict(count=0, param=NULL), STEP_BAD),
    ("null accumulator", dict(accs=_accs(P, NULL)), STEP_ACC),
    ("no adam, null accumulator", dict(adam=0, exp_avg=NULL, exp_avg_sq=NULL, accs=_accs(NULL, P)), STEP_ACC),
    # the first of two
    ("act > 2, null accumulator", dict(act=3, accs=_accs(P, NULL)), STEP_BAD),
]


@pytest.mark.parametrize("what,over,message", STEP, ids=[c[0].replace(" ", "-") for c in STEP])
def test_param_step_refusals(pkg, what, over, message):
    assert _step(pkg._native.lib(), **over) == (INVALID, message)


def test_param_step_with_nothing_to_do(pkg):
    """count 0 returns before the accumulators are looked at."""
    L = pkg._native.lib()
    assert _step(L, count=0)[0] == OK
    assert _step(L, count=0, accs=_accs(P, NULL))[0] == OK
    assert _step(L, count=0, adam=0, exp_avg=NULL, exp_avg_sq=NULL)[0] == OK


def _entry(pkg, **over):
    e = pkg._native.GrParamStep()
    e.count, e.act, e.num_accs, e.param, e.grad, e.exp_avg, e.exp_avg_sq = 10, 2, 2, P, P, P, P
    e.accs[0] = e.accs[1] = P
    e.reg, e.neg_step_size, e.bias_correction2_sqrt = 0.0, -1e-3, 0.5
    accs = over.pop("accs", None)
    for k, v in over.items():
        setattr(e, k, v)
    if accs is not None:
        for j, x in enumerate(accs):
            e.accs[j] = x
    return e


def _steps(pkg, entry, num, entries, sched=(P, P, P, P)):
    L = pkg._native.lib()
    arr = (pkg._native.GrParamStep * max(1, len(entries)))(*entries) if entries is not None else None
    if entry == "gr_fit_param_steps":
        got = L.gr_fit_param_steps(num, arr, B1, B2, EPS, NULL)
    else:
        got = L.gr_fit_param_steps_sched(num, arr, B1, B2, EPS, *sched, NULL)
    return got, L.gr_last_error().decode()


def _steps_cases(pkg):
    good, empty = _entry(pkg), _entry(pkg, count=0)
    cases = [
        ("num < 0", -1, [good], STEPS_BAD),
        ("num > GR_FIT_MAX_PARAMS", 9, [good] * 9, STEPS_BAD),
        ("entries without a list", 1, None, STEPS_BAD),
        ("null accumulator", 1, [_entry(pkg, accs=[P, NULL])], STEPS_ACC),
        ("null accumulator of an empty tensor", 1, [_entry(pkg, count=0, accs=[NULL, P])], STEPS_ACC),
        # the first of two: entry by entry, and within an entry its fields before its accumulators
        ("null accumulator, then a bad entry", 2, [_entry(pkg, accs=[P, NULL]), _entry(pkg, act=3)], STEPS_ACC),
        ("empty, then a bad entry", 2, [empty, _entry(pkg, param=NULL)], STEPS_ENTRY),
        ("bad entry with a null accumulator", 1, [_entry(pkg, act=3, accs=[NULL, P])], STEPS_ENTRY),
    ]
    for what, over in [("count < 0", dict(count=-1)), ("act < 0", dict(act=-1)), ("act > 2", dict(act=3)),
                       ("null param", dict(param=NULL)), ("null exp_avg", dict(exp_avg=NULL)),
                       ("null exp_avg_sq", dict(exp_avg_sq=NULL)), ("num_accs < 0", dict(num_accs=-1)),
                       ("num_accs > GR_FIT_MAX_ACC", dict(num_accs=9))]:
        cases.append((what, 1, [_entry(pkg, **over)], STEPS_ENTRY))
        cases.append((what + ", second entry", 2, [good, _entry(pkg, **over)], STEPS_ENTRY))
    return cases


@pytest.mark.parametrize("entry", ["gr_fit_param_steps", "gr_fit_param_steps_sched"])
def test_param_steps_refusals(pkg, entry):
    """Both batched entries refuse with gr_fit_param_steps' texts (they share their checks)."""
    cases = _steps_cases(pkg)
    assert len(cases) >= 24
    for what, num, entries, message in cases:
        assert _steps(pkg, entry, num, entries) == (INVALID, message), what


def test_param_steps_sched_refusals(pkg):
    """Its own operands come first; pinned memory is asked for only after the entries passed (no entry with elements
    here: with one, the update is launched before that check)."""
    good, empty = _entry(pkg), _entry(pkg, count=0)
    for k in range(4):
        sched = tuple(NULL if j == k else P for j in range(4))
        assert _steps(pkg, "gr_fit_param_steps_sched", 1, [good], sched) == (INVALID, SCHED_NULL), k
        assert _steps(pkg, "gr_fit_param_steps_sched", -1, [_entry(pkg, act=3)], sched) == (INVALID, SCHED_NULL), k
    assert _steps(pkg, "gr_fit_param_steps_sched", 2, [empty, empty]) == (INVALID, SCHED_PINNED)
    assert _steps(pkg, "gr_fit_param_steps_sched", 0, None) == (INVALID, SCHED_PINNED)
    assert _steps(pkg, "gr_fit_param_steps_sched", 2, [empty, _entry(pkg, act=3)]) == (INVALID, STEPS_ENTRY)


def test_param_steps_with_nothing_to_do(pkg):
    empty = _entry(pkg, count=0)
    assert _steps(pkg, "gr_fit_param_steps", 0, None)[0] == OK
    assert _steps(pkg, "gr_fit_param_steps", 0, [empty])[0] == OK
    assert _steps(pkg, "gr_fit_param_steps", 3, [empty] * 3)[0] == OK


ADAM = [("count < 0", dict(count=-1)), ("null param", dict(param=NULL)), ("null grad", dict(grad=NULL)),
        ("null exp_avg", dict(exp_avg=NULL)), ("null exp_avg_sq", dict(exp_avg_sq=NULL)),
        ("count 0, null grad", dict(count=0, grad=NULL))]


@pytest.mark.parametrize("what,over", ADAM, ids=[c[0].replace(" ", "-") for c in ADAM])
def test_adam_step_refusals(pkg, what, over):
    L = pkg._native.lib()
    a = dict(count=10, param=P, grad=P, exp_avg=P, exp_avg_sq=P)
    a.update(over)
    got = L.gr_adam_step(a["count"], a["param"], a["grad"], a["exp_avg"], a["exp_avg_sq"], -1e-3, 0.5, B1, B2, EPS, NULL)
    assert (got, L.gr_last_error().decode()) == (INVALID, ADAM_BAD)
    assert L.gr_adam_step(0, P, P, P, P, -1e-3, 0.5, B1, B2, EPS, NULL) == OK
