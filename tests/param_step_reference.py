"""TEST INFRASTRUCTURE ONLY: the fit loop's parameter update in float64, with a bar for every element of every output.

The contract restated (include/gr_hip.h, "Fit-loop parameter update"), evaluated on the float32 inputs widened to
float64 with the scalars as the float32 values the library receives (``scalars``):

* gradient stage, from ``(x, accs, reg)``: ``S = sum(accs) + reg``, ``A = sum(|accs|) + |reg|`` (the same sum with every
  term taken absolutely, as tests/pergaussian_reference.py does), ``g = act'(x) S`` with the true derivatives
  (identity 1; softplus sigma(x); sigmoid sigma(x) (1 - sigma(x))) -- ``gradient``;
* Adam stage, from ``(g32, p, m, v)`` where g32 is the gradient the library wrote, an exact float32 input:
  ``m' = m + w1 (g - m)``, ``v' = w2 g^2 + b2 v`` -- ``moments``; ``p' = p + ns m' / (sqrt(v') / bc + eps)`` from the
  library's own float32 m' and v' -- ``param``.  Each stage's bar then covers that stage's roundings only.

The bars, one term per rounding, u = 2^-24 (half an ulp, relative), na accumulators:

  identity   (na + 1) u A
  softplus   A ((na + C_SUM) u sigma + e^-20 [x > 20]) + 2^-126 A + 2^-126
  sigmoid    A u ((na + C_SUM) sigma' + C_Y sigma |1 - 2 sigma|) + 2^-126 A + 2^-126
  m'         u (C_M w1 |g - m| + |m'|) + 2^-149
  v'         C_V u v' + 4 2^-149
  p'         u (|p'| + C_P |update|) + 2^-149

* the accumulator sum takes na roundings of at most u A each; the product with the activation's derivative, the
  denominator ``z + 1`` / ``1 + e`` and the division one each.  ``expf`` is taken at EXPF_ULP = 2 ulp = 4 u relative (the
  HIP math documentation's figure is not to hand; 2 ulp is the assumption): through z / (z + 1) it arrives as
  4 u (1 - sigma), so softplus needs na + 3 + 4 = na + 7, and C_SUM = 7.  In the sigmoid y = 1 / (1 + e) is off by
  u (2 + 4 (1 - sigma)) relative, and (1 - y) y turns that into sigma |1 - 2 sigma| u (2 + 4 (1 - sigma)), which is at
  most 2 u sigma |1 - 2 sigma| + 4 u sigma'; with the rounding of 1 - y and the two products (3 u sigma'), na + 7 and
  C_Y >= 2.  C_Y stays 4.
* e^-20 is torch's threshold: for x > 20 the backward returns g, not g sigma(x), and 1 - sigma(x) < e^-x < e^-20.
* the sigma |1 - 2 sigma| term is y's own rounding carried through torch's formula g (1 - y) y: at x >~ 10 it exceeds
  sigma' itself (at x >= 17, 1 + e^-x rounds to 1 and the gradient is exactly 0).  Design precision, not a defect.
* the two 2^-126 terms: ``expf`` and the product in the subnormal range, whether or not they are flushed.
* m': the rounding of g - m (u w1 |g - m|, C_M = 2 leaves one to spare) and of the result; v': g g, v b2 and the result;
  p': sqrt, / bc, + eps and the quotient (4 u |update|, C_P = 6) and the result.  2^-149: a result in the subnormal
  range.  There is no other absolute floor: an element whose bar is 0 must be exactly 0, and every output is finite.

Domain: ``|g| <= 1e18`` (beyond it g^2 leaves float32's range, as it does in torch) and ``eps > 0``.

``emulate`` is the kernel's operation order in float32 numpy (fused multiply-adds through float64), with one
injectable defect: what tests/test_param_step_ref_cpu.py shows the bars to reject.  ``data`` / ``adam_data`` build the
inputs of both test files.
"""
from __future__ import annotations

import math

import numpy as np

F = np.float32
U = 2.0 ** -24
TINY, DENORM = 2.0 ** -126, 2.0 ** -149
E20 = math.exp(-20.0)
EXPF_ULP = 2  # assumed (see above)
C_SUM, C_Y, C_M, C_V, C_P = 7, 4, 2, 3, 6  # the issue's 5, 4, 2, 3, 6: C_SUM raised for a 2-ulp expf, the rest as stated
IDENTITY, SOFTPLUS, SIGMOID = 0, 1, 2
ACT_NAMES = ("identity", "softplus", "sigmoid")
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-15
G_MAX = 1e18


def scalars(t, lr=LR, b1=B1, b2=B2, eps=EPS):
    """The float32 scalars the library receives for update t (the eager step's two expressions, then 1 - beta1, beta2,
    1 - beta2 rounded from double, and eps): dict of Python floats holding float32 values."""
    u = float(t)
    return {"ns": float(F(-(lr / (1.0 - b1 ** u)))), "bc": float(F((1.0 - b2 ** u) ** 0.5)), "w1": float(F(1.0 - b1)),
            "b2": float(F(b2)), "w2": float(F(1.0 - b2)), "eps": float(F(eps))}


def _wide(a):
    a = np.asarray(a)
    assert a.dtype == F, a.dtype
    return a.astype(np.float64)


def _sigma(x):
    """sigma(x) in float64 without cancellation on either side."""
    with np.errstate(under="ignore", over="ignore"):
        e = np.exp(-np.abs(x))
    return np.where(x >= 0.0, 1.0 / (1.0 + e), e / (1.0 + e))


def gradient(act, x, accs, reg):
    """(g, bar, A) of the gradient stage: float64 arrays of x's shape.  reg: the float32 value the library receives."""
    x = _wide(x)
    r = float(F(reg))
    S, A = np.full_like(x, r), np.full_like(x, abs(r))
    for a in accs:
        S, A = S + _wide(a), A + np.abs(_wide(a))
    na = len(accs)
    if act == IDENTITY:
        return S, (na + 1) * U * A, A
    sg = _sigma(x)
    if act == SOFTPLUS:
        return sg * S, A * ((na + C_SUM) * U * sg + E20 * (x > 20.0)) + TINY * A + TINY, A
    assert act == SIGMOID
    d = sg * _sigma(-x)
    return d * S, A * U * ((na + C_SUM) * d + C_Y * sg * np.abs(1.0 - 2.0 * sg)) + TINY * A + TINY, A


def moments(g32, m, v, sc):
    """((m', bar), (v', bar)) from the gradient the library wrote and the state before."""
    g, m, v = _wide(g32), _wide(m), _wide(v)
    assert np.all(np.abs(g) <= G_MAX), "outside the domain: |g| <= 1e18"
    m1 = m + sc["w1"] * (g - m)
    v1 = sc["w2"] * g * g + sc["b2"] * v
    return (m1, U * (C_M * sc["w1"] * np.abs(g - m) + np.abs(m1)) + DENORM), (v1, C_V * U * v1 + 4 * DENORM)


def param(p, m1_32, v1_32, sc):
    """(p', bar) from the library's own float32 m' and v'."""
    assert sc["eps"] > 0.0, "outside the domain: eps > 0"
    p, m1, v1 = _wide(p), _wide(m1_32), _wide(v1_32)
    upd = sc["ns"] * m1 / (np.sqrt(v1) / sc["bc"] + sc["eps"])
    p1 = p + upd
    return p1, U * (np.abs(p1) + C_P * np.abs(upd)) + DENORM


def ratios(got, ref, bar):
    """|got - ref| / bar per element: 0 where both vanish, inf where the bar is 0 and got differs, or got is not finite."""
    got = np.asarray(got)
    assert got.dtype == F and got.shape == ref.shape, (got.dtype, got.shape, ref.shape)
    err = np.abs(got.astype(np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bar > 0.0, err / bar, np.where(err > 0.0, np.inf, 0.0))
    return np.where(np.isfinite(got), r, np.inf)


def assert_within(got, ref, bar, what):
    """Every element finite and within its bar (exactly the reference where the bar is 0).  Returns the worst ratio."""
    r = ratios(got, ref, bar)
    if r.size == 0:
        return 0.0
    i = int(np.argmax(r))
    worst = float(r.reshape(-1)[i])
    if not worst <= 1.0:
        gv, rv, bv = (np.asarray(a).reshape(-1)[i] for a in (got, ref, bar))
        raise AssertionError(f"{what}: |got - ref| / bar = {worst:.3e} at element {i} (got {gv!r}, reference {rv!r}, "
                             f"bar {bv!r})")
    return worst


def check_gradient(act, x, accs, reg, g32, what):
    g, bar, _ = gradient(act, x, accs, reg)
    return {"g": assert_within(g32, g, bar, f"{what}: g")}


def check_adam(g32, p, m, v, sc, p1, m1, v1, what):
    """The Adam stage's three outputs within their bars: {"m": ratio, "v": ratio, "p": ratio}."""
    (mr, mb), (vr, vb) = moments(g32, m, v, sc)
    pr, pb = param(p, m1, v1, sc)
    return {"m": assert_within(m1, mr, mb, f"{what}: m'"), "v": assert_within(v1, vr, vb, f"{what}: v'"),
            "p": assert_within(p1, pr, pb, f"{what}: p'")}


# ---------------------------------------------------------------------------------------------------------------------
# The data of both test files
# ---------------------------------------------------------------------------------------------------------------------
_EDGES = [20.0, 19.999998, 20.000002, -104.0, 88.0, -88.0, 103.0, 87.0, -87.0, 88.7, -88.7, 0.0, 15.0, -15.0, 17.0, 30.0,
          -30.0]
_EDGES_SIGMOID = [-88.7, 88.0, 17.0, -104.0, 103.0, 88.7, -88.0, 87.0, -87.0, 15.0, -15.0, 30.0, -30.0, 0.0, 20.0, 19.999998,
                  20.000002]
REG = (0.0, 1e-4, 2e-6)  # per activation (identity without accumulators: a bar of 0, a gradient of exactly 0)


def _state(rng, n, t):
    """m = v = 0 before update 1; else m ~ 1e-3 N(0, 1), v ~ 1e-6 U with every fifth exactly 0 and every ninth subnormal."""
    if t == 1:
        return np.zeros(n, F), np.zeros(n, F)
    m = (1e-3 * rng.standard_normal(n)).astype(F)
    v = (1e-6 * rng.random(n)).astype(F)
    v[2::5] = 0.0
    v[4::9] = F(1e-40)
    return m, v


def data(n, act, na, t, seed=0):
    """(x, m, v, accs) for the fused entries: x with the activation's edges first (softplus: both sides of its threshold
    20; sigmoid: the tails where expf overflows or 1 - y cancels), so that a count of 1, 3 or 4 still sees one, then
    6 N(0, 1); accumulators of magnitudes log-uniform over 1e-6 .. 1e2 and random sign, every seventh element with
    acc1 = -acc0 (1 + 2^-20).  The first n elements of a longer array of the same arguments are the same elements."""
    rng = np.random.default_rng([seed, act, na, t])
    big = max(n, 2048)
    x = (6.0 * rng.standard_normal(big)).astype(F)
    edge = np.array(_EDGES_SIGMOID if act == SIGMOID else _EDGES, F)
    x[:edge.size] = edge
    accs = []
    for _ in range(na):
        mag = 10.0 ** rng.uniform(-6.0, 2.0, big)
        accs.append((mag * np.where(rng.random(big) < 0.5, -1.0, 1.0)).astype(F))
    if na >= 2:
        accs[1][::7] = -(accs[0][::7] * F(1.0 + 2.0 ** -20))
    m, v = _state(rng, big, t)
    return x[:n].copy(), m[:n].copy(), v[:n].copy(), [a[:n].copy() for a in accs]


def benign_data(n, na, seed=0):
    """(x, m, v, accs) of the kind the fitter tests run on (x ~ 3 N(0, 1), accumulators ~ N(0, 1), m ~ 1e-3 N(0, 1),
    v ~ 1e-6 U > 0): no threshold, no tail, no cancellation.  What an aggregate check of the parameters sees."""
    rng = np.random.default_rng([seed, 7, na])
    x = (3.0 * rng.standard_normal(n)).astype(F)
    m = (1e-3 * rng.standard_normal(n)).astype(F)
    v = (1e-6 * (0.01 + rng.random(n))).astype(F)
    return x, m, v, [rng.standard_normal(n).astype(F) for _ in range(na)]


def adam_data(n, t, seed=0):
    """(p, g, m, v) for gr_adam_step: |g| log-uniform over 1e-25 .. 1e17 (g g underflows below ~1e-23), every eleventh
    exactly 0, and after update 1 every thirteenth m = g (1 + 2^-21) (g - m cancels)."""
    rng = np.random.default_rng([seed, 99, t])
    big = max(n, 2048)
    p = (3.0 * rng.standard_normal(big)).astype(F)
    g = (10.0 ** rng.uniform(-25.0, 17.0, big) * np.where(rng.random(big) < 0.5, -1.0, 1.0)).astype(F)
    g[3::11] = 0.0
    m, v = _state(rng, big, t)
    if t > 1:
        m[5::13] = g[5::13] * F(1.0 + 2.0 ** -21)
    return p[:n].copy(), g[:n].copy(), m[:n].copy(), v[:n].copy()


# ---------------------------------------------------------------------------------------------------------------------
# The kernel's operation order in float32, with one injectable defect
# ---------------------------------------------------------------------------------------------------------------------
DEFECTS = ("softplus_threshold_2", "first_pass_only", "bias_correction_of_t_minus_1", "eps_inside_sqrt",
           "eighth_accumulator_dropped", "one_minus_y_is_1_above_15")
FIRST_PASS = 4096 * 256


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def emulate_gradient(act, x, accs, reg, defect=None):
    """act_backward on the accumulators summed in order plus reg, float32."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        use = accs[:7] if defect == "eighth_accumulator_dropped" else accs
        s = use[0].copy() if use else np.zeros_like(x)
        for a in use[1:]:
            s = s + a
        s = s + F(reg)
        if act == SOFTPLUS:
            z = np.exp(x)
            return np.where(x > F(2.0 if defect == "softplus_threshold_2" else 20.0), s, s * z / (z + F(1.0))).astype(F)
        if act == SIGMOID:
            y = F(1.0) / (F(1.0) + np.exp(-x))
            w = F(1.0) - y
            if defect == "one_minus_y_is_1_above_15":
                w = np.where(x > F(15.0), F(1.0), w)
            return (s * w * y).astype(F)
        return s.astype(F)


def emulate_adam(g, p, m, v, sc, defect=None):
    """adam_elem, float32: (p', m', v')."""
    ns, bc, w1, b2, w2, eps = (F(sc[k]) for k in ("ns", "bc", "w1", "b2", "w2", "eps"))
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        m1 = _fma(w1, g - m, m)
        v1 = _fma(w2, g * g, v * b2)
        den = np.sqrt(v1 + eps) / bc if defect == "eps_inside_sqrt" else np.sqrt(v1) / bc + eps
        p1 = _fma(ns, m1 / den, p)
    if defect == "first_pass_only":
        p1[FIRST_PASS:], m1[FIRST_PASS:], v1[FIRST_PASS:] = p[FIRST_PASS:], m[FIRST_PASS:], v[FIRST_PASS:]
    return p1, m1, v1
