"""CPU: the refusals of the view backward's entries that return before any device call (gr_bwd, gr_bwd_indexed,
gr_bwd_l1, gr_bwd_fit, gr_bwd_fit_gather, gr_bwd_fit_ssim, gr_bwd_fit_ssim_gather, and the two other entries that build a
view loss, gr_fwd_render_l1 and gr_fit_views_batched): each with the status and the exact gr_last_error() text, and where
two refusals apply the one that comes first.  The expected strings are written out here (from the source as it was
before the entries filled a request struct), never read from the library.  No pointer is dereferenced."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

INVALID, WORKSPACE = 1, 3  # GR_ERR_INVALID_ARGUMENT, GR_ERR_WORKSPACE
N = 10

NULL_VIEW = "view is null"
NULL_PLAN = "plan is null"
DEPTH = "depth gradient for a view rendered with no_depth_grad (render it with depth_grad=True)"
TILE32 = "32-pixel tiles (gr_view.tile = 32): the fused fit path only (gr_bwd_splat)"
ROWS = "a band of tile rows (gr_view.rows): the fused fit path only (gr_bwd_splat)"
COLOR_DIM = "colors must be (N,3) or SH coeffs (N,4,3) / (N,16,3)"
NULL_POINTER = "null pointer"
NULL_LOSS = "gr_bwd_l1: null loss or workspace"
WS_SMALL = "backward workspace too small"
FWD_L1_VIEW = "gr_fwd_render_l1: the view must have no_depth_grad = 1 or 2"
FWD_L1_WS = "gr_fwd_render_l1: backward workspace too small (or null loss)"

_BUF = (ctypes.c_float * 4)()
P = ctypes.cast(_BUF, ctypes.c_void_p)  # a non-null pointer (never dereferenced)
NULL = ctypes.c_void_p(0)
F = ctypes.c_float


def _defaults(pkg, depth_grad=True):
    """The named operands of a call that passes every check up to the first launch (which no case reaches)."""
    nat = pkg._native
    gv = pkg.torch_renderer.make_view(np.eye(4, dtype="float32"), np.eye(4, dtype="float32"), 40, 24, depth_grad=depth_grad)
    return dict(view=gv, plan=nat.GrPlan(100, 200, 100), cd=3, up=P, g_depth=NULL, target=P, mask=NULL, tdepth=NULL, loss=P,
                sums=P, w_dssim=0.2, ws_bytes=1 << 40)


def _head(a):
    return [ctypes.byref(a["view"]) if a["view"] is not None else None, N,
            ctypes.byref(a["plan"]) if a["plan"] is not None else None]


def _params(a):
    return [P, P, P, a["cd"], P]


def _loss(a, depth=True, ssim=False):
    return ([a["target"], a["mask"], F(0.2)] + ([a["tdepth"], F(0.05)] if depth else []) + [F(0.25)]
            + ([F(a["w_dssim"])] if ssim else []) + [a["loss"]])


STATE, GRADS = [P, P, P], [P, P, P, P]

# entry -> its argument list from the named operands (the header's order)
CALLS = {
    "gr_bwd": lambda a: _head(a) + _params(a) + STATE + [a["up"], P, a["g_depth"]] + GRADS + [P, a["ws_bytes"], NULL],
    "gr_bwd_indexed": lambda a: (_head(a) + _params(a) + STATE + [a["up"], P, a["g_depth"]] + [P] + GRADS
                                 + [P, a["ws_bytes"], NULL]),
    "gr_bwd_l1": lambda a: _head(a) + _params(a) + STATE + _loss(a, depth=False) + GRADS + [0, P, a["ws_bytes"], NULL],
    "gr_bwd_fit": lambda a: _head(a) + _params(a) + STATE + _loss(a) + GRADS + [1, P, a["ws_bytes"], NULL],
    "gr_bwd_fit_gather": lambda a: _head(a) + STATE + _loss(a) + [P, a["ws_bytes"], a["sums"], P, NULL],
    "gr_bwd_fit_ssim": lambda a: _head(a) + _params(a) + STATE + _loss(a, ssim=True) + GRADS + [0, P, a["ws_bytes"], NULL],
    "gr_bwd_fit_ssim_gather": lambda a: _head(a) + STATE + _loss(a, ssim=True) + [P, a["ws_bytes"], a["sums"], P, NULL],
    "gr_fwd_render_l1": lambda a: (_head(a) + [P, P, 1 << 40, P, 1 << 40] + _loss(a, depth=False) + [NULL, NULL]
                                   + [P, a["ws_bytes"], NULL]),
}
BACKWARD = [e for e in CALLS if e != "gr_fwd_render_l1"]
WITH_PARAMS = ["gr_bwd", "gr_bwd_indexed", "gr_bwd_l1", "gr_bwd_fit", "gr_bwd_fit_ssim"]
FIT = [e for e in BACKWARD if e not in ("gr_bwd", "gr_bwd_indexed")]
WITH_DEPTH = ["gr_bwd_fit", "gr_bwd_fit_gather", "gr_bwd_fit_ssim", "gr_bwd_fit_ssim_gather"]
GATHER = ["gr_bwd_fit_gather", "gr_bwd_fit_ssim_gather"]
SSIM = ["gr_bwd_fit_ssim", "gr_bwd_fit_ssim_gather"]


def _view_with(pkg, a, **fields):
    v = pkg._native.GrView.from_buffer_copy(a["view"])
    for k, val in fields.items():
        setattr(v, k, val)
    return v


def _cases(pkg):
    """(entry, what, operand overrides, status, message)."""
    out = []
    base = _defaults(pkg)
    flat = _defaults(pkg, depth_grad=False)  # no_depth_grad = 1
    assert base["view"].no_depth_grad == 0 and flat["view"].no_depth_grad == 1
    for e in BACKWARD:
        out.append((e, "null view", dict(view=None), INVALID, NULL_VIEW))
        out.append((e, "null plan", dict(plan=None), INVALID, NULL_PLAN))
        out.append((e, "tile 32", dict(view=_view_with(pkg, base, tile=32)), INVALID, TILE32))
        out.append((e, "rows > 0", dict(view=_view_with(pkg, base, rows=1)), INVALID, ROWS))
        out.append((e, "workspace one byte short", dict(ws_bytes=None), WORKSPACE, WS_SMALL))
        # the first of two: the view before the plan, the tile before the rows and the plan, the plan before the colours
        out.append((e, "null view, null plan", dict(view=None, plan=None), INVALID, NULL_VIEW))
        out.append((e, "tile 32, rows > 0, null plan", dict(view=_view_with(pkg, base, tile=32, rows=1), plan=None), INVALID, TILE32))
        out.append((e, "rows > 0, null plan", dict(view=_view_with(pkg, base, rows=1), plan=None), INVALID, ROWS))
    for e in WITH_PARAMS:
        for cd in (0, 4, 16):
            out.append((e, f"color_dim {cd}", dict(cd=cd), INVALID, COLOR_DIM))
        out.append((e, "null plan, bad color_dim", dict(plan=None, cd=5), INVALID, NULL_PLAN))
    for e in ("gr_bwd", "gr_bwd_indexed"):
        out.append((e, "no upstream image gradient", dict(up=NULL), INVALID, NULL_POINTER))
        out.append((e, "g_depth, no_depth_grad view", dict(view=flat["view"], g_depth=P), INVALID, DEPTH))
        out.append((e, "g_depth, no_depth_grad view, tile 32", dict(view=_view_with(pkg, flat, tile=32), g_depth=P), INVALID, DEPTH))
    for e in FIT:
        out.append((e, "null target_rgb", dict(target=NULL), INVALID, f"{e}: target_rgb is null"))
        out.append((e, "null target_rgb, null view", dict(target=NULL, view=None), INVALID, f"{e}: target_rgb is null"))
        out.append((e, "null loss", dict(loss=NULL), INVALID, NULL_LOSS))
        out.append((e, "null loss, bad workspace", dict(loss=NULL, ws_bytes=0), INVALID, NULL_LOSS))
    for e in WITH_DEPTH:
        out.append((e, "depth target, no_depth_grad view", dict(view=flat["view"], tdepth=P), INVALID, DEPTH))
        out.append((e, "depth target, no_depth_grad view, null plan", dict(view=flat["view"], tdepth=P, plan=None), INVALID, DEPTH))
    for e in GATHER:
        out.append((e, "null sums", dict(sums=NULL), INVALID, f"{e}: sums is null"))
        out.append((e, "null target_rgb, null sums", dict(target=NULL, sums=NULL), INVALID, f"{e}: target_rgb is null"))
        out.append((e, "null sums, null view", dict(sums=NULL, view=None), INVALID, f"{e}: sums is null"))
    for e in SSIM:
        for lam in (1.5, -0.25, float("nan")):
            out.append((e, f"w_dssim {lam}", dict(w_dssim=lam), INVALID, f"{e}: w_dssim must be in [0, 1]"))
        out.append((e, "null target_rgb, w_dssim 2", dict(target=NULL, w_dssim=2.0), INVALID, f"{e}: target_rgb is null"))
        out.append((e, "w_dssim 2, null view", dict(w_dssim=2.0, view=None), INVALID, f"{e}: w_dssim must be in [0, 1]"))
        # a D-SSIM entry needs gr_bwd_ssim_bytes whatever its weight: gr_bwd_bytes is too small at w_dssim = 0 too
        out.append((e, "gr_bwd_bytes at w_dssim 0", dict(w_dssim=0.0, ws_bytes="gr_bwd_bytes"), WORKSPACE, WS_SMALL))
    out.append(("gr_bwd_fit_ssim_gather", "null sums, w_dssim 2", dict(sums=NULL, w_dssim=2.0), INVALID,
                "gr_bwd_fit_ssim_gather: sums is null"))
    e = "gr_fwd_render_l1"
    out.append((e, "null view", dict(view=None), INVALID, FWD_L1_VIEW))
    out.append((e, "no_depth_grad 0", dict(view=base["view"]), INVALID, FWD_L1_VIEW))
    out.append((e, "null target_rgb", dict(target=NULL), INVALID, f"{e}: target_rgb is null"))
    out.append((e, "no_depth_grad 0, null target_rgb", dict(view=base["view"], target=NULL), INVALID, FWD_L1_VIEW))
    out.append((e, "null plan", dict(plan=None), INVALID, NULL_PLAN))
    out.append((e, "null loss", dict(loss=NULL), WORKSPACE, FWD_L1_WS))
    out.append((e, "workspace one byte short", dict(ws_bytes=None), WORKSPACE, FWD_L1_WS))
    out.append((e, "null plan, null loss", dict(plan=None, loss=NULL), INVALID, NULL_PLAN))
    return out


@pytest.mark.parametrize("entry", list(CALLS))
def test_every_refusal_has_its_status_and_text(pkg, entry):
    L = pkg._native.lib()
    cases = [c for c in _cases(pkg) if c[0] == entry]
    assert len(cases) >= 8
    for _, what, over, status, message in cases:
        a = _defaults(pkg, depth_grad=entry != "gr_fwd_render_l1")
        a.update(over)
        ssim = entry in SSIM
        size = L.gr_bwd_ssim_bytes if ssim else L.gr_bwd_bytes
        if a["view"] is not None and a["plan"] is not None:
            need = size(ctypes.byref(a["view"]), N, ctypes.byref(a["plan"]))
            if a["ws_bytes"] is None:
                a["ws_bytes"] = need - 1
            elif a["ws_bytes"] == "gr_bwd_bytes":
                a["ws_bytes"] = L.gr_bwd_bytes(ctypes.byref(a["view"]), N, ctypes.byref(a["plan"]))
                assert a["ws_bytes"] < need
        got = getattr(L, entry)(*CALLS[entry](a))
        text = L.gr_last_error().decode()
        assert (got, text) == (status, message), (entry, what)


def _batch_view(pkg, **over):
    nat = pkg._native
    a = _defaults(pkg, depth_grad=False)
    b = nat.GrBatchView()
    b.view, b.plan = a["view"], a["plan"]
    big = 1 << 40
    b.geom = b.bins = b.scratch = b.ws = b.target_rgb = b.sums = b.loss = P.value
    b.bins_bytes = b.scratch_bytes = b.ws_bytes = big
    for k, v in over.items():
        setattr(b, k, v)
    return b


BATCHED = [
    ("no view", 0, N, {}, INVALID, "gr_fit_views_batched: num_views must be in [1, GR_BATCH_MAX_VIEWS]"),
    ("too many views", 9, N, {}, INVALID, "gr_fit_views_batched: num_views must be in [1, GR_BATCH_MAX_VIEWS]"),
    ("n = 0", 1, 0, {}, INVALID, "gr_fit_views_batched: n must be > 0"),
    ("no view, n = 0", 0, 0, {}, INVALID, "gr_fit_views_batched: num_views must be in [1, GR_BATCH_MAX_VIEWS]"),
    ("null target_rgb", 1, N, dict(target_rgb=None), INVALID, "gr_fit_views_batched: null pointer"),
    ("null loss", 1, N, dict(loss=None), INVALID, "gr_fit_views_batched: null pointer"),
    ("null sums", 1, N, dict(sums=None), INVALID, "gr_fit_views_batched: null pointer"),
    ("depth target without saved sums", 1, N, dict(target_depth=P.value), INVALID, "gr_fit_views_batched: null pointer"),
    ("small backward workspace", 1, N, dict(ws_bytes=16), WORKSPACE, "gr_fit_views_batched: a workspace is too small"),
    ("null loss, small workspace", 1, N, dict(loss=None, ws_bytes=16), INVALID, "gr_fit_views_batched: null pointer"),
    ("depth target, no_depth_grad view", 1, N, dict(target_depth=P.value, saved=P.value, sums3=P.value), INVALID,
     "gr_fit_views_batched: depth loss needs no_depth_grad = 0, the L1 path 1"),
]


@pytest.mark.parametrize("what,num_views,n,over,status,message", BATCHED, ids=[c[0].replace(" ", "-") for c in BATCHED])
def test_batched_entry_refusals(pkg, what, num_views, n, over, status, message):
    L = pkg._native.lib()
    arr = (pkg._native.GrBatchView * max(1, num_views))(*[_batch_view(pkg, **over) for _ in range(max(1, num_views))])
    got = L.gr_fit_views_batched(num_views, arr, n, F(0.2), F(0.05), F(0.25), NULL)
    assert (got, L.gr_last_error().decode()) == (status, message)
