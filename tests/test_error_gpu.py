"""GPU: the blend-weighted pixel error per Gaussian.  Kernel level: gr_error_view (k_error_view + k_error_gather) on a
forward_native state against the float64 dense reference (tests/error_reference.py) within its derived tolerance
|got - ref| <= 1e-4 ref + delta B + o exp(-cutoff^2 / 2) S; the partition of the view's L1 error; the zero-error target;
accumulation over views, view orders and streams bit for bit; the argument checks.  Fitter level:
ViewShardedFitter.error_state through the native executor and through the Python schedule, against per-view calls and
the reference, a fit left unchanged, and densify_and_prune(mode="error")."""
from __future__ import annotations

import ctypes
import importlib

import numpy as np
import pytest
import torch

import error_reference as er

pytestmark = pytest.mark.gpu

FW, FH, FV, FN = 64, 48, 4, 300  # the fitter tests' shape
BG = (0.2, 0.5, 0.7)


@pytest.fixture(scope="module")
def mods(pkg, cuda):
    return (importlib.import_module("3dgaussian_amd.torch_renderer"), importlib.import_module("3dgaussian_amd.fit_multiview"))


_SCENES: dict = {}
_REFS: dict = {}
_TARGETS: dict = {}


def _scene(cuda, n, sigma):
    """(host tensors, device tensors) of er.scene, made once and left unchanged."""
    key = (n, sigma)
    if key not in _SCENES:
        host = er.scene(n, seed=n, sigma=sigma)
        _SCENES[key] = (host, tuple(t.to(cuda).contiguous() for t in host))
    return _SCENES[key]


def _target(cuda, W, H, view=1):
    """A random target in [0, 1]: (host, device)."""
    key = (W, H, view)
    if key not in _TARGETS:
        t = torch.rand((H, W, 3), generator=torch.Generator().manual_seed(100 * W + H + view))
        _TARGETS[key] = (t, t.to(cuda).contiguous())
    return _TARGETS[key]


def _cams(mods, W, H):
    return mods[1].orbit_cameras(3, W, H, "cpu")


def _ref(mods, cuda, W, H, n, sigma, view=1):
    """er.error_ref of the case, computed once: (ref, B, S, out, Wt)."""
    key = (W, H, n, sigma, view)
    if key not in _REFS:
        (m, s, c, o), _ = _scene(cuda, n, sigma)
        cam = _cams(mods, W, H)[view]
        _REFS[key] = er.error_ref(m, s, c, o, cam.view, cam.proj, W, H, _target(cuda, W, H, view)[0], torch.tensor(BG))
    return _REFS[key]


def _render(mods, cuda, W, H, n, sigma, view=1, chunk=0, images=False):
    """(Prepared, RenderState, image) of one view as evaluate() renders it (16-pixel tiles, the 7-sigma footprint)."""
    tr = mods[0]
    _, (m, s, c, o) = _scene(cuda, n, sigma)
    cam = _cams(mods, W, H)[view]
    gv = tr.make_view(cam.view, cam.proj, W, H, torch.tensor(BG), depth_grad=False)
    gv.chunk = chunk
    pv = tr.prepare_native(m, s, c, o, gv)
    out, _, _, rs = tr.forward_native(m, s, c, o, gv, pv, images=images)
    return pv, rs, out


def _err(mods, cuda, W, H, n, sigma, view=1, chunk=0, into=None, target=None, images=False):
    pv, rs, out = _render(mods, cuda, W, H, n, sigma, view, chunk, images)
    err = torch.zeros((n + er.DEAD,), device=cuda) if into is None else into
    mods[0].error_view_native(rs, pv, _target(cuda, W, H, view)[1] if target is None else target, err)
    return err, rs, out


def _compose(mods, rs):
    """The image gr_fwd_compose writes from the state's saved sums."""
    nat = mods[0]._native
    dev = rs.saved.device
    H, W = rs.gv.height, rs.gv.width
    out = torch.empty((H, W, 3), device=dev)
    alpha, depth = torch.empty((H, W), device=dev), torch.empty((H, W), device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    nat.check(nat.lib().gr_fwd_compose(ctypes.byref(rs.gv), nat.ptr(rs.saved), nat.ptr(out), nat.ptr(alpha), nat.ptr(depth),
                                       stream), "gr_fwd_compose")
    return out


CASES = [
    # W, H, n, sigma, chunk
    (17, 13, 1, 0.05, 0),      # one ragged tile, a single Gaussian
    (17, 13, 7, 0.05, 0),
    (64, 48, 257, 0.05, 0),    # not a multiple of the block
    (64, 48, 300, 0.05, 0),
    (200, 120, 2000, 0.3, 0),  # big sigma: ragged in y, tail-only tiles, tiles split over work items
    (200, 120, 2000, 0.3, 64),  # gr_view.chunk = 64: 64-pair work items
]


@pytest.mark.parametrize("W,H,n,sigma,chunk", CASES, ids=[f"{c[0]}x{c[1]}-n{c[2]}" + (f"-chunk{c[4]}" if c[4] else "") for c in CASES])
def test_kernel_matches_reference_and_conserves(mods, cuda, W, H, n, sigma, chunk):
    """Against the reference within the derived tolerance (worst ratio observed: see DESIGN 8i), and the partition
    sum_i got_i + sum_p e r = sum_p e with e, r in float64 from the composed image and the saved W: a pair counted
    twice across split tiles, or lost, breaks it."""
    tr = mods[0]
    err, rs, image = _err(mods, cuda, W, H, n, sigma, chunk=chunk, images=True)
    torch.cuda.synchronize()
    (_, _, _, o), _ = _scene(cuda, n, sigma)
    ref, B, S, out64, _ = _ref(mods, cuda, W, H, n, sigma)
    cutoff = tr.default_cutoff(False)
    assert rs.gv.cutoff == cutoff and rs.plan.num_pairs > 0
    if sigma > 0.1:
        assert rs.plan.num_pairs > rs.plan.num_core_pairs > 0  # tail pairs exist
        tiles = ((W + 15) // 16) * ((H + 15) // 16)
        assert rs.plan.num_pairs > tiles * (chunk or 512)  # (and tiles are split over several work items)
    delta = float((image.double().cpu() - out64).abs().max())  # the existing render against float64
    assert delta < 1e-4  # (the project's parity bar: the render is sound)
    got = err.double().cpu()
    tol = er.tolerance(ref, B, S, o, cutoff, delta)
    ratio = er.worst_ratio(got, ref, tol)
    live = ref > 1e-9
    rel = float(((got - ref).abs()[live] / ref[live]).max())
    # the partition, on the device's own image and weight sums
    t64 = _target(cuda, W, H)[0].double()
    x = _compose(mods, rs).double().cpu()
    assert torch.equal(x, image.double().cpu())
    Wt = rs.saved[:4 * W * H].view(H, W, 4)[..., 0].double().cpu()
    e = (x - t64).abs().sum(-1) / 3.0
    r = 1.0 / (1.0 + Wt)
    lhs, rhs = float(got.sum()) + float((e * r).sum()), float(e.sum())
    print(f"error {W}x{H} n={n} chunk={chunk}: pairs {rs.plan.num_pairs} (core {rs.plan.num_core_pairs}), delta {delta:.2e}, worst "
          f"|got - ref| / tolerance {ratio:.3f}, worst relative error {rel:.2e}, err in [{float(got[:n].min()):.2e}, "
          f"{float(got.max()):.2e}]; partition: {lhs:.6f} against {rhs:.6f} ({abs(lhs - rhs) / float(tol.sum()):.3f} of the "
          f"summed tolerance {float(tol.sum()):.2e})")
    assert bool(((got - ref).abs() <= tol).all())
    assert bool((err[-er.DEAD:] == 0).all())  # behind the camera, off screen, opacity 0, negative opacity: exactly 0
    assert float(err[:n].min()) > 0.0
    assert abs(lhs - rhs) <= float(tol.sum())


def test_zero_error_target(mods, cuda):
    """The target equal to the image gr_fwd_compose writes from the same saved sums: every err_i is exactly 0."""
    W, H, n, sigma = 200, 120, 2000, 0.3
    pv, rs, _ = _render(mods, cuda, W, H, n, sigma)
    image = _compose(mods, rs)
    assert float(image.min()) >= 0.0 and float(image.std()) > 0.01
    err = torch.full((n + er.DEAD,), 0.0, device=cuda)
    mods[0].error_view_native(rs, pv, image, err)
    torch.cuda.synchronize()
    assert not err.any()
    mods[0].error_view_native(rs, pv, (image + 0.25).contiguous(), err)
    assert int((err > 0).sum()) == n


def test_accumulation_order_and_streams(mods, cuda):
    """Three views into one buffer = the elementwise maximum of three one-view calls; reversed order; two streams."""
    W, H, n, sigma = 64, 48, 300, 0.05
    singles = [_err(mods, cuda, W, H, n, sigma, view=v)[0] for v in range(3)]
    want = torch.stack(singles).max(dim=0).values
    assert not torch.equal(singles[0], singles[1])
    for order in ((0, 1, 2), (2, 1, 0)):
        buf = torch.zeros((n + er.DEAD,), device=cuda)
        for v in order:
            _err(mods, cuda, W, H, n, sigma, view=v, into=buf)
        assert torch.equal(buf, want), order
    buf = torch.zeros((n + er.DEAD,), device=cuda)
    for v in range(3):  # (the targets are made on the main stream first)
        _target(cuda, W, H, v)
    main = torch.cuda.current_stream(cuda)
    streams = [torch.cuda.Stream(cuda), torch.cuda.Stream(cuda)]
    for st in streams:
        st.wait_stream(main)
    for v in range(3):
        with torch.cuda.stream(streams[v % 2]):
            _err(mods, cuda, W, H, n, sigma, view=v, into=buf)
    for st in streams:
        main.wait_stream(st)
    torch.cuda.synchronize()
    assert torch.equal(buf, want)
    # a second call on a filled buffer changes nothing
    _err(mods, cuda, W, H, n, sigma, view=1, into=buf)
    assert torch.equal(buf, want)


def test_argument_checks_launch_nothing(mods, cuda):
    tr = mods[0]
    nat = tr._native
    L = nat.lib()
    W, H, n, sigma = 64, 48, 300, 0.05
    pv, rs, _ = _render(mods, cuda, W, H, n, sigma)
    target = _target(cuda, W, H)[1]
    need = int(L.gr_error_ws_bytes(ctypes.byref(rs.gv), rs.n, ctypes.byref(rs.plan)))
    assert need >= 4 * rs.plan.num_pairs
    ws = torch.zeros((need,), dtype=torch.uint8, device=cuda)
    err = torch.zeros((rs.n,), device=cuda)
    stream = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    empty = nat.GrPlan(0, 0, 0)

    def call(gv=rs.gv, nn=rs.n, plan=rs.plan, geom=pv.geom, bins=rs.bins, saved=rs.saved, tgt=target, out=err, wsp=ws,
             ws_bytes=need):
        return L.gr_error_view(ctypes.byref(gv), nn, ctypes.byref(plan), nat.ptr(geom), nat.ptr(bins), nat.ptr(saved),
                               nat.ptr(tgt), nat.ptr(out), nat.ptr(wsp), ws_bytes, stream)

    for field, value in (("tile", 32), ("rows", 1), ("device_counts", 1)):
        bad = nat.GrView.from_buffer_copy(rs.gv)
        setattr(bad, field, value)
        assert call(bad) == nat.GR_ERR_INVALID_ARGUMENT, field
    for kw in (dict(geom=None), dict(bins=None), dict(saved=None), dict(tgt=None), dict(out=None), dict(wsp=None)):
        assert call(**kw) == nat.GR_ERR_INVALID_ARGUMENT, kw
    assert call(ws_bytes=need - 1) == nat.GR_ERR_WORKSPACE and b"workspace" in L.gr_last_error()
    with pytest.raises(ValueError):
        tr.error_view_native(rs, pv, target, err[:-1])
    with pytest.raises(ValueError):
        tr.error_view_native(rs, pv, target[:-1], err)
    assert call(nn=0) == nat.GR_OK and call(plan=empty) == nat.GR_OK and call(plan=empty, wsp=None, ws_bytes=0) == nat.GR_OK
    torch.cuda.synchronize()
    assert not err.any() and not ws.any()  # refusals and no-ops launch nothing
    assert call() == nat.GR_OK
    torch.cuda.synchronize()
    assert int((err > 0).sum()) == n and ws.any()


# ---- fitter level ----------------------------------------------------------------------------------------------------
def _raw_params(cuda):
    """The 64 x 48 scene as the fitter's raw parameters (softplus / sigmoid inverted).  The dead rows: behind the camera,
    off screen and opacity 0 (sigmoid(-200) is 0 in float32); a sigmoid cannot give a negative opacity, that row is
    left out."""
    m, s, c, o = er.scene(FN, seed=FN, sigma=0.05)
    m, s, c, o = m[:-1], s[:-1], c[:-1], o[:-1]
    raw_o = torch.logit(o.clamp(1e-6, 1.0 - 1e-6))
    raw_o[-1] = -200.0
    p = {"means": m, "scales_raw": torch.log(torch.expm1(s - 1e-3)), "opacities_raw": raw_o,
         "colors_raw": torch.logit(c.clamp(0.02, 0.98))}
    return {k: torch.nn.Parameter(v.to(cuda).contiguous()) for k, v in p.items()}


@pytest.fixture(scope="module")
def views(mods, cuda):
    fm = mods[1]
    cams = fm.orbit_cameras(FV, FW, FH, cuda)
    g = torch.Generator(device=cuda).manual_seed(9)
    targets = [torch.rand((FH, FW, 3), generator=g, device=cuda) for _ in cams]
    return cams, targets


def _with(fm, **kw):
    saved = {k: getattr(fm, k) for k in kw}
    for k, v in kw.items():
        setattr(fm, k, v)
    return saved


def test_fitter_error_state(mods, cuda, views):
    tr, fm = mods
    cams, targets = views
    got = {}
    for native in ("1", "0"):
        saved = _with(fm, NATIVE_EXEC=native, NUM_STREAMS=3)
        try:
            f = fm.ViewShardedFitter(_raw_params(cuda), cams, targets, FW, FH)
            f.step()
            assert f.perm is not None and f._native_exec() == (native == "1")
            got[native] = f.error_state()
        finally:
            _with(fm, **saved)
    n = FN + er.DEAD - 1
    assert got["1"].dtype == torch.float32 and tuple(got["1"].shape) == (n,)
    assert torch.equal(got["1"], got["0"])  # the executor and the Python schedule
    with torch.no_grad():
        # the maximum over one-view calls on the fitter's own (Morton) order, put back into canonical order
        m, s, c, o = (t.detach().float().contiguous() for t in f._eval_activations(cuda))
        one, delta = [], 0.0
        cm, cs, cc, co = (t.detach().cpu() for t in fm.activations(f.canonical_params()))
        for cam, t in zip(cams, targets):
            gv = f._eval_view(cam, cuda)
            pv = tr.prepare_native(m, s, c, o, gv)
            _, _, _, rs = tr.forward_native(m, s, c, o, gv, pv, images=False)  # (as error_state renders it)
            image = tr.forward_native(m, s, c, o, gv, pv, images=True, want_depth=False)[0]
            buf = torch.zeros((n,), device=cuda)
            tr.error_view_native(rs, pv, t, buf)
            one.append(buf)
            ref_image = er.cref.render(cm, cs, cc, co, cam.view.cpu(), cam.proj.cpu(), FW, FH)[0]
            delta = max(delta, float((image.double().cpu() - ref_image).abs().max()))
        own = torch.stack(one).max(dim=0).values
        want = torch.empty_like(own)
        want[f.perm] = own
        assert torch.equal(got["1"], want)
        assert torch.equal(f.error_state([cams[2]], [targets[2]])[f.perm], one[2])
        with pytest.raises(ValueError):
            f.error_state(cams)
        with pytest.raises(ValueError):  # a target the kernel cannot read through its pointer: no other form here
            f.error_state([cams[2]], [targets[2].double()])
        ref, B, S = er.error_ref_views(cm, cs, cc, co, [(cam.view.cpu(), cam.proj.cpu()) for cam in cams], FW, FH,
                                       [t.cpu() for t in targets])
    cutoff = tr.default_cutoff(False)
    tol = er.tolerance(ref, B, S, co, cutoff, delta)
    ratio = er.worst_ratio(got["1"].double().cpu(), ref, tol)
    print(f"error_state {FW}x{FH}, {FV} views, n={n}: delta {delta:.2e}, worst |got - ref| / tolerance {ratio:.3f}")
    assert delta < 1e-4  # (the project's parity bar: the render is sound)
    assert bool(((got["1"].double().cpu() - ref).abs() <= tol).all())
    assert bool((got["1"][-(er.DEAD - 1):] == 0).all()) and float(got["1"][:FN].min()) > 0.0


def _same(a, b) -> bool:
    """Bit equality of two results: tensors, or evaluate()'s dicts of float64 arrays and floats."""
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a)
    return torch.equal(a, b)


@pytest.mark.parametrize("streams", [None, 1], ids=["streams-default", "streams-1"])
def test_passes_share_the_executor_workspace(mods, cuda, views, streams):
    """evaluate(), contribution_state() and error_state() interleaved on one fitter through the native executor, whose
    streams keep one workspace for whichever pass runs (the metrics' partial sums and the pairs' values differ in
    size): every repeated call gives the bits of its first, and each result those of a fresh fitter that made only
    that call."""
    _, fm = mods
    cams, targets = fm.orbit_cameras(3, FW, FH, cuda), views[1][:3]
    saved = _with(fm, NATIVE_EXEC="1", **({} if streams is None else {"NUM_STREAMS": streams}))
    try:
        def fitter():
            f = fm.ViewShardedFitter(_raw_params(cuda), cams, targets, FW, FH)
            f.step()
            assert f._native_exec()
            return f

        f = fitter()
        order = ("evaluate", "contribution_state", "error_state", "contribution_state", "evaluate", "error_state")
        first = {}
        for name in order:
            got = getattr(f, name)()
            assert _same(got, first.setdefault(name, got)), name
        for name, got in first.items():
            assert _same(getattr(fitter(), name)(), got), name
        assert float(first["contribution_state"].max()) > 0.0 and float(first["error_state"].max()) > 0.0
        assert not torch.equal(first["contribution_state"], first["error_state"]) and first["evaluate"]["mean_l1"] > 0.0
    finally:
        _with(fm, **saved)


@pytest.mark.parametrize("native", ["1", "0"], ids=["executor", "python"])
def test_error_state_does_not_change_the_fit(mods, cuda, views, native):
    """Three steps against one step, error_state(), two steps: losses, parameters and Adam moments bit for bit."""
    _, fm = mods
    cams, targets = views
    saved = _with(fm, NATIVE_EXEC=native)
    try:
        runs = []
        for ask in (False, True):
            f = fm.ViewShardedFitter(_raw_params(cuda), cams, targets, FW, FH)
            losses = [f.step()]
            if ask:
                grads = {k: v.grad.detach().clone() for k, v in f.params.items()}
                before = {k: v.detach().clone() for k, v in f.params.items()}
                assert float(f.error_state().max()) > 0.0
                for k, v in f.params.items():
                    assert torch.equal(v.grad, grads[k]) and torch.equal(v.detach(), before[k]), k
            losses += [f.step() for _ in range(2)]
            torch.cuda.synchronize()
            runs.append(([float(x) for x in losses], {k: v.detach().clone() for k, v in f.params.items()},
                         {k: (f.opt.state[v]["exp_avg"].clone(), f.opt.state[v]["exp_avg_sq"].clone()) for k, v in f.params.items()}))
    finally:
        _with(fm, **saved)
    a, b = runs
    assert a[0] == b[0], (a[0], b[0])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
        assert torch.equal(a[2][k][0], b[2][k][0]) and torch.equal(a[2][k][1], b[2][k][1]), k


@pytest.mark.parametrize("prune_mode", ["opacity", "contribution"])
def test_densify_mode_error_on_the_device(mods, cuda, views, prune_mode):
    """densify_and_prune(mode="error") gives the rows of densify_by_error applied to error_state() by hand (with
    prune_mode="contribution": on the rows prune_by_contribution keeps), on a fitter without density_stats, and the
    step after it runs."""
    _, fm = mods
    cams, targets = views
    f = fm.ViewShardedFitter(_raw_params(cuda), cams, targets, FW, FH, density_stats=False)
    f.step()
    err = f.error_state()
    n = err.shape[0]
    keep, thr = None, 1.0 / 510.0
    if prune_mode == "contribution":
        peak = f.contribution_state()
        thr = float(peak.sort().values[60])
        keep = fm.prune_by_contribution(peak, thr)
        kept = int(keep.sum())
    else:
        kept = int((torch.sigmoid(f.canonical_params()["opacities_raw"].detach()) > 0.05).sum())
    assert 64 <= kept < n
    split_scale = float((torch.nn.functional.softplus(f.params["scales_raw"].detach()) + 1e-3)[:, :2].max(dim=1).values.median())
    gen = torch.Generator(device=cuda).manual_seed(f.densify_seed)
    rep = {}
    want = fm.densify_by_error(f.canonical_params(), err, 0.0, split_scale, 1000, 0.05, int(kept * 0.15), gen, keep=keep,
                               report=rep)
    f.densify_and_prune(1000, 0.15, 0.05, mode="error", split_scale=split_scale, prune_mode=prune_mode, prune_contribution=thr)
    after = f.canonical_params()
    assert rep["clones"] > 0 and rep["splits"] > 0 and after["means"].shape[0] == kept + int(kept * 0.15)
    for k in want:
        assert torch.equal(after[k].detach(), want[k].detach()), k
    r = f.error_report
    assert r["n"] == n and r["clones"] == rep["clones"] and r["splits"] == rep["splits"] and r["max"] == float(err.max())
    loss = f.step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(torch.as_tensor(loss)))
    assert f.error_state().shape[0] == kept + int(kept * 0.15)
