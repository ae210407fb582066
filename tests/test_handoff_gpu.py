"""GPU: the cross-workgroup hand-offs inside a launch, pinned directly at small work items and under load.

A tile whose pair list is longer than the work-item length is split over several workgroups; each leaves its partial
sums with write-through stores and takes the tile's ticket (arrive_last), the last to arrive sums them.  The same
pattern carries the view loss (arrive_last_tile), the column scan's fan-in that builds the work items, k_pixel_grads,
k_depth_tile_max / k_depth_tile_sums, k_ssim_pixel_grads and the regulariser of k_fit_activations.  On
tests/handoff_reference.py's piled scene (one tile of ~80 items beside empty and one-item tiles at 64-pair items):

a. the work-item lists of every builder (the counting sort's fan-in, k_work_items, the batched forms; host- and
   device-sized views) equal handoff_reference.work_items bit for bit;
b. every consumer leaves the whole ticket region zero, and a second render through the same bins without re-binning
   is bit-identical;
c. every kernel family that consumes work items meets the project's bars against the float64 binned oracle at work-item
   lengths 64, 192 and the default, and each split tile taken alone is within 1e-3 (one partial of a tile of
   m <= 84 items missing or stale moves that tile by ~1/m >= 1.2e-2; the kernels' documented 2^-16 is 60x below);
d. images of 1, 2, 4, 6, 8 and 9 tiles (arrive_last_of with fewer than, exactly and more than eight arrivals);
e. 24 launches of the batched call alternating two colour sets through the same buffers while two other streams
   render something else: every word of the losses, the per-Gaussian sums and the images equals the idle device's
   single-view results; likewise the regulariser of gr_fit_activations through one workspace.

Measured on an MI355X (profiles/handoff_tests.txt): (c) images <= 2.0e-6, loss <= 3.1e-8, gradients <= 9.5e-6, the worst
split tile 8.8e-5 (a two-item tile of the mode without depth; 5e-6 elsewhere); (d) loss <= 7.6e-8; (e) 4 x 11,213,016
words and the regulariser's 24: no mismatch, with 62 to 100 % of the launches' time overlapped by the other streams'
renders.  With the partial sums of a split tile summed over one item less, every case of (c) fails (depth 1.2e-3 against
2e-5); without the last arriver's ticket reset, (a) and (b) fail.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import handoff_reference as hr
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

W, H = 112, 80
CHUNKS = (64, 192, 0)
ONE_ZONE = 5.0  # the fit path's footprint (one zone, 5 sigma)
TWO_ZONES = (7.0, 5.5)


class Env:
    def __init__(self, pkg, dev):
        self.tr, self.nat, self.dev = pkg.torch_renderer, pkg._native, dev
        self.L = self.nat.lib()
        self.scene = hr.piled_scene()
        self.t = [torch.from_numpy(a).to(dev).contiguous() for a in self.scene.arrays()]
        self.n = int(self.t[0].shape[0])
        rng = np.random.default_rng(17)
        self.colors_b = rng.random((self.n, 3)).astype(np.float32)  # the second colour set of (e)

    def stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)


@pytest.fixture(scope="module")
def env(pkg, cuda):
    return Env(pkg, cuda)


def _cam(W, H, k=1, of=4):
    return orc.orbit_cameras(of, W, H)[k]


def _gv(env, cam, W, H, zones, tile=0, chunk=0, ndg=1):
    """zones: ONE_ZONE or TWO_ZONES; ndg: gr_view.no_depth_grad (0 f32-grade with a depth gradient, 1 two-piece, 2
    f32-grade without)."""
    cutoff, core = (zones, zones) if isinstance(zones, float) else zones
    gv = env.tr.make_view(cam[0], cam[1], W, H, None, cutoff=cutoff, core_cutoff=core, depth_grad=ndg == 0, tile=tile)
    gv.no_depth_grad = ndg
    gv.chunk = chunk
    return gv


def _oview(cam, W, H, zones, tile=0):
    cutoff, core = (zones, zones) if isinstance(zones, float) else zones
    return orc.make_view(cam[0], cam[1], W, H, None, cutoff=cutoff, core_cutoff=core, tile=tile)


_ORACLE: dict = {}


def _oracle_fwd(env, cam_key, W, H, zones, tile=0, colors=None):
    """(out, alpha, depth, ranges) of the float64 binned oracle, computed once per view and left unchanged."""
    key = ("fwd", cam_key, W, H, zones, tile, colors is not None)
    if key not in _ORACLE:
        sc = env.scene if colors is None else orc.Scene(env.scene.means, env.scene.scales, colors, env.scene.opacities)
        v = _oview(_cam(W, H, *cam_key), W, H, zones, tile)
        rec, rect, counts = orc.preprocess(v, sc)
        _ORACLE[key] = orc.forward(v, sc, binned=True) + (orc.bin_pairs(v, rec, rect, counts)[3],)
    return _ORACLE[key]


def _oracle_bwd(env, cam_key, W, H, zones, tile, g_rgb, g_alpha, g_depth, colors=None):
    key = ("bwd", cam_key, W, H, zones, tile, colors is not None, g_rgb.tobytes(), g_alpha.tobytes(),
           None if g_depth is None else g_depth.tobytes())
    if key not in _ORACLE:
        sc = env.scene if colors is None else orc.Scene(env.scene.means, env.scene.scales, colors, env.scene.opacities)
        v = _oview(_cam(W, H, *cam_key), W, H, zones, tile)
        _ORACLE[key] = orc.backward(v, sc, g_rgb, g_alpha, g_depth, binned=True)
    return _ORACLE[key]


# ---- low-level calls that keep every workspace --------------------------------------------------------------------
class Bufs:
    """One view's workspaces, sized by its plan (counts, or capacities for a device-sized view)."""

    def __init__(self, env, gv, plan, geom=None, fill=None):
        L, n, r = env.L, env.n, ctypes.byref
        self.gv, self.plan, self.geom = gv, plan, geom

        def mk(nbytes):
            if fill is None:
                return torch.empty((int(nbytes),), dtype=torch.uint8, device=env.dev)
            return torch.full((int(nbytes),), fill, dtype=torch.uint8, device=env.dev)

        if geom is None:
            self.geom = mk(L.gr_geom_bytes(n))
        self.bins = mk(L.gr_bins_bytes(r(gv), n, r(plan)))
        self.scratch = mk(L.gr_fwd_scratch_bytes(r(gv), n, r(plan)))
        self.ws = mk(L.gr_bwd_bytes(r(gv), n, r(plan)))


def _binned(env, gv):
    b = env.nat.GrView.from_buffer_copy(gv)
    b.binned = 1
    return b


def _prepare(env, gv, t=None):
    """(geom, plan) of a host-sized view."""
    p = env.tr.prepare_native(*(t or env.t), gv)
    return p.geom, p.plan()


def _prepare_sized(env, gv, plan, t=None):
    """The view device-sized with capacities about 1.5x its counts: (gr_view, geom, capacities)."""
    nat = env.nat
    gvs = nat.GrView.from_buffer_copy(gv)
    gvs.device_counts = 1
    caps = _caps(nat, plan)
    observed = torch.zeros(3, dtype=torch.int64, pin_memory=True)
    overflow = torch.zeros(1, dtype=torch.int32, device=env.dev)
    p = env.tr.prepare_views_sized(*(t or env.t), [gvs], [caps], [observed], overflow)[0]
    torch.cuda.synchronize()
    assert int(overflow) == 0 and observed.tolist()[0] == plan.num_pairs and observed.tolist()[2] == plan.num_core_pairs
    return gvs, p.geom, caps


def _caps(nat, plan):
    kc, kt = int(plan.num_core_pairs), int(plan.num_pairs - plan.num_core_pairs)
    cc, ct = (3 * kc + 1) // 2, (3 * kt + 1) // 2
    return nat.GrPlan(cc + ct, cc + ct, cc)


def _fwd_render(env, b, gv=None, out=None, alpha=None, depth=None, saved=None):
    nat, r = env.nat, ctypes.byref
    nat.check(env.L.gr_fwd_render(r(gv or b.gv), env.n, r(b.plan), nat.ptr(b.geom), nat.ptr(b.bins), b.bins.numel(),
                                  nat.ptr(b.scratch), b.scratch.numel(), nat.ptr(out), nat.ptr(alpha), nat.ptr(depth),
                                  nat.ptr(saved), env.stream()), "gr_fwd_render")


def _fwd_l1(env, b, target, mask, w_sil, g_scale, loss, gv=None, out=None, alpha=None):
    nat, r = env.nat, ctypes.byref
    nat.check(env.L.gr_fwd_render_l1(r(gv or b.gv), env.n, r(b.plan), nat.ptr(b.geom), nat.ptr(b.bins), b.bins.numel(),
                                     nat.ptr(b.scratch), b.scratch.numel(), nat.ptr(target), nat.ptr(mask),
                                     ctypes.c_float(w_sil), ctypes.c_float(g_scale), nat.ptr(loss), nat.ptr(out),
                                     nat.ptr(alpha), nat.ptr(b.ws), b.ws.numel(), env.stream()), "gr_fwd_render_l1")


def _grads(env):
    return tuple(torch.empty_like(x) for x in env.t)


def _bwd(env, b, saved, g_out, g_alpha, g_depth, grads):
    nat, r = env.nat, ctypes.byref
    m, s, c, o = env.t
    nat.check(env.L.gr_bwd(r(b.gv), env.n, r(b.plan), nat.ptr(m), nat.ptr(s), nat.ptr(c), 3, nat.ptr(o), nat.ptr(b.geom),
                           nat.ptr(b.bins), nat.ptr(saved), nat.ptr(g_out), nat.ptr(g_alpha), nat.ptr(g_depth),
                           *(nat.ptr(g) for g in grads), nat.ptr(b.ws), b.ws.numel(), env.stream()), "gr_bwd")


def _bwd_fit(env, b, saved, target, mask, w_sil, dtarget, w_depth, g_scale, loss, grads, w_dssim=None):
    nat, r, L = env.nat, ctypes.byref, env.L
    m, s, c, o = env.t
    head = (r(b.gv), env.n, r(b.plan), nat.ptr(m), nat.ptr(s), nat.ptr(c), 3, nat.ptr(o), nat.ptr(b.geom), nat.ptr(b.bins),
            nat.ptr(saved), nat.ptr(target), nat.ptr(mask), ctypes.c_float(w_sil), nat.ptr(dtarget), ctypes.c_float(w_depth),
            ctypes.c_float(g_scale))
    if w_dssim is None:
        nat.check(L.gr_bwd_fit(*head, nat.ptr(loss), *(nat.ptr(g) for g in grads), 0, nat.ptr(b.ws), b.ws.numel(),
                               env.stream()), "gr_bwd_fit")
        return b.ws
    ws = torch.empty((int(L.gr_bwd_ssim_bytes(r(b.gv), env.n, r(b.plan))),), dtype=torch.uint8, device=env.dev)
    nat.check(L.gr_bwd_fit_ssim(*head, ctypes.c_float(w_dssim), nat.ptr(loss), *(nat.ptr(g) for g in grads), 0,
                                nat.ptr(ws), ws.numel(), env.stream()), "gr_bwd_fit_ssim")
    return ws


def _batch_entry(env, e, b, target, mask, sums, loss, saved=None, dtarget=None, sums3=None):
    e.view, e.plan = b.gv, b.plan
    e.geom, e.bins, e.bins_bytes = b.geom.data_ptr(), b.bins.data_ptr(), b.bins.numel()
    e.scratch, e.scratch_bytes = b.scratch.data_ptr(), b.scratch.numel()
    e.ws, e.ws_bytes = b.ws.data_ptr(), b.ws.numel()
    e.saved = saved.data_ptr() if saved is not None else None
    e.target_rgb = target.data_ptr()
    e.target_mask = mask.data_ptr() if mask is not None else None
    e.target_depth = dtarget.data_ptr() if dtarget is not None else None
    e.sums = sums.data_ptr()
    e.sums3 = sums3.data_ptr() if sums3 is not None else None
    e.loss = loss.data_ptr()


def _batched(env, arr, w_sil, w_depth, g_scale):
    env.nat.check(env.L.gr_fit_views_batched(len(arr), arr, env.n, ctypes.c_float(w_sil), ctypes.c_float(w_depth),
                                             ctypes.c_float(g_scale), env.stream()), "gr_fit_views_batched")


def _tiles(gv):
    te = 32 if gv.tile == 32 else 16
    return te, ((gv.width + te - 1) // te) * ((gv.height + te - 1) // te)


def _lists(env, b):
    """The work-item part of a view's bins, read back: ranges, items (the whole capacity), num_items, tile_item0, the
    ticket region and the work-item length."""
    nat = env.nat
    K = int(b.plan.num_pairs)
    off, ch = nat.items_layout(b.gv, env.n, K)
    roff = nat.bins_layout(b.gv, env.n, K)[2]
    _, tiles = _tiles(b.gv)
    raw = b.bins.cpu().numpy()
    cap = (K + ch - 1) // ch + 2 * tiles

    def ints(o, count):
        return raw[o:o + 4 * count].view(np.int32)

    assert off == sorted(off) and all(o % 256 == 0 for o in off) and off[3] + 4 * hr.ticket_words(tiles) <= raw.shape[0]
    assert off[1] - off[0] >= 16 * cap and off[3] - off[2] >= 8 * tiles
    return dict(ranges=ints(roff, 4 * tiles).reshape(2 * tiles, 2), items=ints(off[0], 4 * cap).reshape(cap, 4),
                num=ints(off[1], 2), item0=ints(off[2], 2 * tiles), ticket=ints(off[3], hr.ticket_words(tiles)), ch=ch,
                tiles=tiles)


def _check_lists(env, b, chunk, two_zones, uneven=True):
    torch.cuda.synchronize()
    d = _lists(env, b)
    assert d["ch"] == (chunk if chunk else d["ch"]) and d["ch"] % 64 == 0
    if not chunk:
        assert d["ch"] >= 512  # the default rule's floor (chunk_of)
    hr.compare_items(d["items"], d["num"], d["item0"], d["ranges"], d["ch"])
    hr.assert_tickets_zero(d["ticket"], d["tiles"])
    if uneven:
        hr.assert_uneven(d["ranges"], two_zones)
    return d


# ---- a. the work-item lists of every builder ----------------------------------------------------------------------
BUILDERS = ["render_two_zones", "l1_t16", "l1_t32", "l1_sized_t16", "l1_sized_t32", "batched_t16", "batched_t32",
            "batched_sized_t16", "batched_sized_t32"]


def _target(env, W, H, seed):
    g = torch.Generator(device=env.dev).manual_seed(seed)
    target = torch.rand((H, W, 3), generator=g, device=env.dev)
    return target, (target.mean(dim=2) > 0.5).float().contiguous()


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("builder", BUILDERS)
def test_work_items_bit_exact(env, builder, chunk):
    """Workspaces start filled with 0xA5 (production allocates them uninitialised): the builders write every word the
    consumers read, the tickets included."""
    tile = 32 if builder.endswith("t32") else 16
    target, mask = _target(env, W, H, 3)
    loss = torch.zeros(8, device=env.dev)
    if builder == "render_two_zones":
        gv = _gv(env, _cam(W, H), W, H, TWO_ZONES, chunk=chunk, ndg=1)
        geom, plan = _prepare(env, gv)
        b = Bufs(env, gv, plan, geom, fill=0xA5)
        saved = torch.empty((5 * W * H,), device=env.dev)
        _fwd_render(env, b, saved=saved)
        d = _check_lists(env, b, chunk, True)
        assert int(d["num"][0]) == int(hr.tile_items(d["ranges"], d["ch"]).sum())
        return
    if builder.startswith("l1"):
        gv = _gv(env, _cam(W, H), W, H, ONE_ZONE, tile=tile, chunk=chunk)
        geom, plan = _prepare(env, gv)
        if "sized" in builder:
            gv, geom, plan = _prepare_sized(env, gv, plan)
        b = Bufs(env, gv, plan, geom, fill=0xA5)
        _fwd_l1(env, b, target, mask, 0.2, 1.0, loss[:1])
        _check_lists(env, b, chunk, False)
        return
    cams = [_cam(W, H, k, 8) for k in range(8)]
    bufs = []
    for cam in cams:
        gv = _gv(env, cam, W, H, ONE_ZONE, tile=tile, chunk=chunk)
        geom, plan = _prepare(env, gv)
        if "sized" in builder:
            gv, geom, plan = _prepare_sized(env, gv, plan)
        else:
            plan = env.nat.GrPlan(plan.num_pairs, max(plan.num_slots, plan.num_pairs), plan.num_core_pairs)
        bufs.append(Bufs(env, gv, plan, geom, fill=0xA5))
    sums = torch.empty((8, env.n, 8), device=env.dev)
    arr = (env.nat.GrBatchView * 8)()
    for j, b in enumerate(bufs):
        _batch_entry(env, arr[j], b, target, mask, sums[j], loss[j:j + 1])
    _batched(env, arr, 0.2, 0.0, 0.125)
    for b in bufs:
        _check_lists(env, b, chunk, False)


@pytest.mark.parametrize("tile", [16, 32])
def test_work_items_empty_view(env, tile):
    """A view without a pair: every tile gets its one empty item (k_work_items), the image is the background.  The
    scene is moved behind the camera: pairs are culled by geometry alone, so zero opacities (still 10,718 pairs at 16
    pixels) do not empty a view."""
    m, s, c, o = env.t
    eye = torch.from_numpy(orc.camera_position(_cam(W, H)[0])).to(env.dev)
    t0 = [(m + 2.0 * eye).contiguous(), s, c, o]
    target, _ = _target(env, W, H, 4)
    for chunk in (64, 0):
        gv = _gv(env, _cam(W, H), W, H, ONE_ZONE, tile=tile, chunk=chunk)
        geom, plan = _prepare(env, gv, t0)
        assert plan.num_pairs == 0
        b = Bufs(env, gv, plan, geom, fill=0xA5)
        loss = torch.zeros(1, device=env.dev)
        out = torch.full((H, W, 3), 7.0, device=env.dev)
        alpha = torch.full((H, W), 7.0, device=env.dev)
        _fwd_l1(env, b, target, None, 0.0, 1.0, loss, out=out, alpha=alpha)
        d = _check_lists(env, b, chunk, False, uneven=False)
        assert d["num"].tolist() == [d["tiles"], 0]
        assert d["items"][:d["tiles"]].tolist() == [[2 * t, 0, 0, 0] for t in range(d["tiles"])]
        assert not out.any() and not alpha.any()
        want = float(target.double().mean())
        assert abs(float(loss) - want) <= 1e-5 * want


@pytest.mark.parametrize("chunk", CHUNKS)
def test_work_items_radix_path(env, chunk):
    """2064 x 1040 = 8,385 tiles: past the counting sort's 8,192, the radix sort's ranges cut by k_work_items over 33
    rounds of its 256-thread block.  Items only."""
    BW, BH = 2064, 1040
    gv = _gv(env, _cam(BW, BH), BW, BH, TWO_ZONES, chunk=chunk)
    geom, plan = _prepare(env, gv)
    b = Bufs(env, gv, plan, geom, fill=0xA5)
    nat, r = env.nat, ctypes.byref
    nat.check(env.L.gr_fwd_bin(r(gv), env.n, r(plan), nat.ptr(geom), nat.ptr(b.bins), b.bins.numel(), nat.ptr(b.scratch),
                               b.scratch.numel(), env.stream()), "gr_fwd_bin")
    d = _check_lists(env, b, chunk, True)
    assert d["tiles"] == 8385 and int(hr.list_lengths(d["ranges"]).sum()) == plan.num_pairs


# ---- b. tickets are left zero; a second render through the same bins ---------------------------------------------------
def _zero_tickets(env, b, what):
    torch.cuda.synchronize()
    d = _lists(env, b)
    try:
        hr.assert_tickets_zero(d["ticket"], d["tiles"])
    except AssertionError as e:
        raise AssertionError(f"after {what}: {e}") from None
    return d


@pytest.mark.parametrize("chunk", [64, 0])
def test_tickets_left_zero_two_zones(env, chunk):
    """gr_fwd_render, gr_fwd_render_saved + gr_fwd_compose, gr_bwd, gr_bwd_fit with a depth target and gr_bwd_fit_ssim
    on one view's bins: after each the tickets and fan-in counters read zero; every repeat is bit-identical."""
    dev = env.dev
    gv = _gv(env, _cam(W, H), W, H, TWO_ZONES, chunk=chunk, ndg=0)
    geom, plan = _prepare(env, gv)
    b = Bufs(env, gv, plan, geom)
    bgv = _binned(env, gv)

    def images():
        return (torch.full((H, W, 3), 9.0, device=dev), torch.full((H, W), 9.0, device=dev),
                torch.full((H, W), 9.0, device=dev), torch.full((5 * W * H,), 9.0, device=dev))

    first = images()
    _fwd_render(env, b, None, *first)
    d = _zero_tickets(env, b, "gr_fwd_render")
    hr.assert_uneven(d["ranges"], True)
    second = images()
    _fwd_render(env, b, bgv, *second)  # binned = 1: nothing re-zeroes the tickets
    _zero_tickets(env, b, "gr_fwd_render (binned)")
    for x, y, name in zip(first, second, ("out", "alpha", "depth", "saved")):
        assert torch.equal(x, y), f"second render through the same bins: {name} differs"
    saved2 = torch.full((5 * W * H,), 9.0, device=dev)
    nat, r = env.nat, ctypes.byref
    nat.check(env.L.gr_fwd_render_saved(r(bgv), env.n, r(plan), nat.ptr(geom), nat.ptr(b.bins), b.bins.numel(),
                                        nat.ptr(b.scratch), b.scratch.numel(), nat.ptr(saved2), env.stream()),
              "gr_fwd_render_saved")
    third = images()[:3]
    nat.check(env.L.gr_fwd_compose(r(gv), nat.ptr(saved2), *(nat.ptr(x) for x in third), env.stream()), "gr_fwd_compose")
    _zero_tickets(env, b, "gr_fwd_render_saved + gr_fwd_compose")
    assert torch.equal(saved2, first[3])
    for x, y, name in zip(first, third, ("out", "alpha", "depth")):
        assert torch.equal(x, y), f"gr_fwd_compose of the saved sums: {name} differs"

    saved = first[3]
    g = torch.Generator(device=dev).manual_seed(21)
    g_out = torch.randn((H, W, 3), generator=g, device=dev)
    g_alpha = torch.randn((H, W), generator=g, device=dev)
    g_depth = torch.randn((H, W), generator=g, device=dev)
    target, mask = _target(env, W, H, 5)
    dtarget = torch.rand((H, W), generator=g, device=dev)
    runs = {
        "gr_bwd": lambda gr, ls: _bwd(env, b, saved, g_out, g_alpha, g_depth, gr),
        "gr_bwd_fit": lambda gr, ls: _bwd_fit(env, b, saved, target, mask, 0.2, dtarget, 0.1, 0.25, ls, gr),
        "gr_bwd_fit_ssim": lambda gr, ls: _bwd_fit(env, b, saved, target, mask, 0.2, dtarget, 0.1, 0.25, ls, gr, w_dssim=0.2),
    }
    for name, run in runs.items():
        got = []
        for _ in range(2):
            grads, loss = _grads(env), torch.full((1,), 9.0, device=dev)
            run(grads, loss)
            _zero_tickets(env, b, name)
            got.append((grads, loss))
        for x, y in zip(got[0][0] + (got[0][1],), got[1][0] + (got[1][1],)):
            assert torch.equal(x, y), f"{name}: the second run through the same bins differs"
        assert all(bool(torch.isfinite(x).all()) and bool(x.any()) for x in got[0][0])
    # and the forward once more after the backwards' fan-ins
    last = images()
    _fwd_render(env, b, bgv, *last)
    _zero_tickets(env, b, "gr_fwd_render after the backwards")
    for x, y in zip(first, last):
        assert torch.equal(x, y)


@pytest.mark.parametrize("tile", [16, 32])
def test_tickets_left_zero_fit_path(env, tile):
    """gr_fwd_render_l1 (the loss fan-in behind the split tiles) twice through one view's bins, then the batched call
    on eight views (the L1 path; at 16-pixel tiles also the depth-loss path): tickets zero, repeats bit-identical."""
    dev = env.dev
    target, mask = _target(env, W, H, 6)
    gv = _gv(env, _cam(W, H), W, H, ONE_ZONE, tile=tile, chunk=64)
    geom, plan = _prepare(env, gv)
    b = Bufs(env, gv, plan, geom)
    got = []
    for k in range(3):
        loss = torch.full((1,), 9.0, device=dev)
        out, alpha = torch.full((H, W, 3), 9.0, device=dev), torch.full((H, W), 9.0, device=dev)
        b.ws.fill_(0xA5)
        _fwd_l1(env, b, target, mask, 0.2, 0.25, loss, gv=_binned(env, gv) if k else None, out=out, alpha=alpha)
        d = _zero_tickets(env, b, f"gr_fwd_render_l1 (run {k})")
        got.append((loss, out, alpha, b.ws.clone()))
    hr.assert_uneven(d["ranges"], False)
    for k in (1, 2):
        for x, y, name in zip(got[0], got[k], ("loss", "out", "alpha", "workspace")):
            assert torch.equal(x, y), f"render {k} through the same bins: {name} differs"

    def batch(depth):
        zones, ndg = (TWO_ZONES, 0) if depth else (ONE_ZONE, 1)
        bufs = []
        for k in range(8):
            v = _gv(env, _cam(W, H, k, 8), W, H, zones, tile=tile, chunk=64, ndg=ndg)
            ge, pl = _prepare(env, v)
            bufs.append(Bufs(env, v, env.nat.GrPlan(pl.num_pairs, max(pl.num_slots, pl.num_pairs), pl.num_core_pairs), ge))
        g = torch.Generator(device=dev).manual_seed(22)
        dtarget = torch.rand((H, W), generator=g, device=dev) if depth else None
        res = []
        for _ in range(2):
            sums = torch.full((8, env.n, 8), 9.0, device=dev)
            sums3 = torch.full((8, env.n), 9.0, device=dev) if depth else None
            saved = torch.empty((8, 5 * W * H), device=dev) if depth else None
            loss = torch.full((8,), 9.0, device=dev)
            arr = (env.nat.GrBatchView * 8)()
            for j, bb in enumerate(bufs):
                _batch_entry(env, arr[j], bb, target, mask, sums[j], loss[j:j + 1], saved[j] if depth else None, dtarget,
                             sums3[j] if depth else None)
            _batched(env, arr, 0.2, 0.1 if depth else 0.0, 0.125)
            for j, bb in enumerate(bufs):
                _zero_tickets(env, bb, f"gr_fit_views_batched (depth={depth}), view {j}")
            res.append((sums, loss) + ((sums3,) if depth else ()))
        for x, y in zip(*res):
            assert torch.equal(x, y) and bool(torch.isfinite(x).all())

    batch(False)
    if tile == 16:
        batch(True)


# ---- c. split tiles against the float64 binned oracle at every work-item length -------------------------------------
def _per_tile(h_out, h_alpha, o_out, o_alpha, ranges, ch, te, W, H):
    """Worst relL2 of out / alpha over one tile taken alone, among the tiles of two or more items: (error, tile, items,
    tiles looked at)."""
    items = hr.tile_items(ranges, ch)
    tx = (W + te - 1) // te
    worst = (0.0, -1, 0)
    split = np.nonzero(items >= 2)[0]
    for t in split:
        sl = (slice((t // tx) * te, min(H, (t // tx) * te + te)), slice((t % tx) * te, min(W, (t % tx) * te + te)))
        e = max(orc.rel_l2(h_out[sl], o_out[sl]), orc.rel_l2(h_alpha[sl], o_alpha[sl]))
        if e > worst[0]:
            worst = (e, int(t), int(items[t]))
    return worst + (len(split),)


def _grad_errs(grads, ora, xy_only):
    errs = {}
    for name, h, o in zip(("d_means", "d_scales", "d_colors", "d_opac"), grads, ora):
        h = h.cpu().numpy()
        if name == "d_scales" and xy_only:  # the fused path's scale gradient has no z column
            h, o = h[:, :2], o[:, :2]
        errs[name] = orc.rel_l2(h, o)
    return errs


def _assert_bars(tag, errs, tile_err):
    print(f"{tag}:", {k: f"{e:.2e}" for k, e in errs.items()},
          f"worst split tile {tile_err[1]} ({tile_err[2]} items, {tile_err[3]} split tiles): {tile_err[0]:.2e}")
    for k, e in errs.items():
        bar = 2e-5 if k in ("out", "alpha", "depth") else 1e-5 if k == "loss" else 1e-4
        assert e <= bar, (tag, k, e, bar)
    assert tile_err[3] >= 1 and tile_err[0] <= 1e-3, (tag, tile_err)


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("family", ["mfma1_depth_grad", "mfma2_depth_output", "mfma3_no_depth"])
def test_split_tiles_render_op(env, family, chunk):
    """k_raster_fwd_mfma<1> / <2> / <3> (forward_native) and k_raster_bwd_bf16 (backward_native, random upstreams, with
    and without a depth gradient) on the two-zone view."""
    tr = env.tr
    ndg = 0 if family.startswith("mfma1") else 1
    want_depth = not family.startswith("mfma3")
    gv = _gv(env, _cam(W, H), W, H, TWO_ZONES, chunk=chunk, ndg=ndg)
    out, alpha, depth, st = tr.forward_native(*env.t, gv, want_depth=want_depth)
    assert (depth is not None) == want_depth
    rng = np.random.default_rng(31)
    g_rgb = rng.standard_normal((H, W, 3)).astype(np.float32)
    g_a = rng.standard_normal((H, W)).astype(np.float32)
    g_d = rng.standard_normal((H, W)).astype(np.float32) if ndg == 0 else None
    dev = env.dev
    grads = tr.backward_native(*env.t, st, torch.from_numpy(g_rgb).to(dev), torch.from_numpy(g_a).to(dev),
                               torch.from_numpy(g_d).to(dev) if g_d is not None else None)
    torch.cuda.synchronize()
    o_out, o_alpha, o_depth, ranges = _oracle_fwd(env, (1, 4), W, H, TWO_ZONES)
    ora = _oracle_bwd(env, (1, 4), W, H, TWO_ZONES, 0, g_rgb, g_a, g_d)
    h_out, h_alpha = out.cpu().numpy(), alpha.cpu().numpy()
    errs = {"out": orc.rel_l2(h_out, o_out), "alpha": orc.rel_l2(h_alpha, o_alpha)}
    if want_depth:
        errs["depth"] = orc.rel_l2(depth.cpu().numpy(), o_depth)
    errs.update(_grad_errs(grads, ora, xy_only=False))
    _, ch = env.nat.items_layout(gv, env.n, st.num_pairs)
    assert ch == (chunk or ch) and int(hr.list_lengths(ranges).sum()) == st.num_pairs
    _assert_bars(f"{family} chunk={chunk} (ch {ch})", errs, _per_tile(h_out, h_alpha, o_out, o_alpha, ranges, ch, 16, W, H))


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("family", ["mfma4_t16", "mfma5_t16_f32_grade", "fwd32_bwd32"])
def test_split_tiles_fit_path(env, family, chunk):
    """k_raster_fwd_mfma<4> / <5> with the 16-pixel fused backward, and k_fwd32_l1 with k_bwd32: forward_l1_native +
    backward_splat_native + gather + reduce_sums_native, the L1 upstream from the HIP images' signs."""
    tr, dev = env.tr, env.dev
    tile = 32 if family == "fwd32_bwd32" else 16
    ndg = 2 if family.startswith("mfma5") else 1
    target, mask = _target(env, W, H, 12)
    w_sil, g_scale, HW = 0.2, 0.25, H * W
    gv = _gv(env, _cam(W, H), W, H, ONE_ZONE, tile=tile, chunk=chunk, ndg=ndg)
    prep = tr.prepare_native(*env.t, gv)
    loss = torch.zeros(1, device=dev)
    out, alpha = torch.empty((H, W, 3), device=dev), torch.empty((H, W), device=dev)
    st, ws = tr.forward_l1_native(*env.t, gv, prep, target, mask, w_sil, g_scale, loss, out=out, alpha=alpha)
    tr.backward_splat_native(st, ws)
    sums = tr.gather_view_native(st, ws)
    grads = _grads(env)
    tr.reduce_sums_native(*env.t, [(st.gv, sums)], grads, accumulate=False)
    torch.cuda.synchronize()
    o_out, o_alpha, _, ranges = _oracle_fwd(env, (1, 4), W, H, ONE_ZONE, tile)
    h_out, h_alpha = out.cpu().numpy().astype(np.float64), alpha.cpu().numpy().astype(np.float64)
    tn, mn = target.cpu().numpy(), mask.cpu().numpy()
    o_loss = np.abs(o_out.astype(np.float64) - tn).mean() + w_sil * np.abs(o_alpha.astype(np.float64) - mn).mean()
    g_rgb = (np.sign(h_out - tn) * (g_scale / (3 * HW))).astype(np.float32)
    g_a = (np.sign(h_alpha - mn) * (w_sil * g_scale / HW)).astype(np.float32)
    ora = _oracle_bwd(env, (1, 4), W, H, ONE_ZONE, tile, g_rgb, g_a, None)
    errs = {"out": orc.rel_l2(h_out, o_out), "alpha": orc.rel_l2(h_alpha, o_alpha), "loss": abs(float(loss) - o_loss) / o_loss}
    errs.update(_grad_errs(grads, ora, xy_only=True))
    _, ch = env.nat.items_layout(gv, env.n, st.num_pairs)
    assert ch == (chunk or ch) and int(hr.list_lengths(ranges).sum()) == st.num_pairs
    _assert_bars(f"{family} chunk={chunk} (ch {ch})", errs, _per_tile(h_out, h_alpha, o_out, o_alpha, ranges, ch, tile, W, H))


# ---- d. small fan-in counts -----------------------------------------------------------------------------------------
SMALL = [(16, 16), (40, 24), (64, 32), (48, 48)]  # 1, 6, 8, 9 tiles of 16 pixels; 1, 2, 2, 4 of 32


def _bwd_ws_parts(env, gv, plan):
    """Byte offsets of (tile_aux, dscal) in the backward workspace (gr_bwd_bytes' layout, restated; the total is
    checked against the library's, so a changed layout fails here and not as a wrong read)."""
    te, tiles = _tiles(gv)
    n = env.n

    def al(x):
        return (x + 255) // 256 * 256

    uf = 2 * 3 * 3 * 64 if te == 16 else 2 * 4 * 2 * 2 * 64 + 64
    o_uf = al(max(int(plan.num_slots), 1) * 9 * 4)
    o_loss = o_uf + al(tiles * uf * 16)
    o_aux = o_loss + al(tiles * 4 * 4)
    o_dscal = o_aux + al(tiles * 2 * 4)
    end = o_dscal + al(16) + al(8 * n * 4) + al(n * 4) + al((n + 255) // 256 * 35 * 8)
    assert end == int(env.L.gr_bwd_bytes(ctypes.byref(gv), n, ctypes.byref(plan)))
    return o_aux, o_dscal


@pytest.mark.parametrize("SW,SH", SMALL, ids=[f"{a}x{b}" for a, b in SMALL])
def test_small_fan_in_counts(env, SW, SH):
    """arrive_last_of with count < 8, = 8 and = 9 and the column scan with two blocks: the view loss of
    gr_fwd_render_l1 (both tile sizes) and of gr_bwd_fit with a depth target against the oracle images' loss in
    float64; the depth maximum and its gradient scalar against numpy on the HIP depth image."""
    dev = env.dev
    target, mask = _target(env, SW, SH, 40 + SW)
    tn, mn = target.cpu().numpy().astype(np.float64), mask.cpu().numpy().astype(np.float64)
    w_sil, w_depth, g_scale = 0.2, 0.1, 0.25
    for tile in (16, 32):
        gv = _gv(env, _cam(SW, SH), SW, SH, ONE_ZONE, tile=tile)
        geom, plan = _prepare(env, gv)
        assert plan.num_pairs > 0
        b = Bufs(env, gv, plan, geom, fill=0xA5)
        loss = torch.full((1,), 9.0, device=dev)
        _fwd_l1(env, b, target, mask, w_sil, g_scale, loss)
        d = _check_lists(env, b, 0, False, uneven=False)
        o_out, o_alpha, _, _ = _oracle_fwd(env, (1, 4), SW, SH, ONE_ZONE, tile)
        want = np.abs(o_out.astype(np.float64) - tn).mean() + w_sil * np.abs(o_alpha.astype(np.float64) - mn).mean()
        print(f"{SW}x{SH} tile {tile}: {d['tiles']} tiles, {int(d['num'][0])} items, "
              f"loss error {abs(float(loss) - want) / want:.2e}")
        assert abs(float(loss) - want) <= 1e-5 * want

    gv = _gv(env, _cam(SW, SH), SW, SH, TWO_ZONES, ndg=0)
    geom, plan = _prepare(env, gv)
    b = Bufs(env, gv, plan, geom, fill=0xA5)
    out, alpha = torch.empty((SH, SW, 3), device=dev), torch.empty((SH, SW), device=dev)
    depth, saved = torch.empty((SH, SW), device=dev), torch.empty((5 * SW * SH,), device=dev)
    _fwd_render(env, b, None, out, alpha, depth, saved)
    g = torch.Generator(device=dev).manual_seed(41)
    dtarget = torch.rand((SH, SW), generator=g, device=dev)
    loss = torch.full((1,), 9.0, device=dev)
    grads = _grads(env)
    _bwd_fit(env, b, saved, target, mask, w_sil, dtarget, w_depth, g_scale, loss, grads)
    d = _check_lists(env, b, 0, True, uneven=False)
    o_out, o_alpha, o_depth, _ = _oracle_fwd(env, (1, 4), SW, SH, TWO_ZONES)
    od, dt = o_depth.astype(np.float64), dtarget.cpu().numpy().astype(np.float64)
    want = (np.abs(o_out.astype(np.float64) - tn).mean() + w_sil * np.abs(o_alpha.astype(np.float64) - mn).mean()
            + w_depth * np.abs(od / (od.max() + 1e-6) - dt).mean())
    err = abs(float(loss) - want) / want
    # the depth scalars: [0] the image's depth maximum, [1] the gradient reaching each arg-max pixel
    o_aux, o_dscal = _bwd_ws_parts(env, gv, plan)
    dscal = b.ws.cpu().numpy()[o_dscal:o_dscal + 8].view(np.float32)
    hd = depth.cpu().numpy()
    M = float(hd.max())
    assert M > 0.0 and abs(float(dscal[0]) - M) <= 5e-7 * M  # (the same float32 quotient, up to a contraction)
    dm = np.float32(dscal[0]) + np.float32(1e-6)
    q = (hd / dm).astype(np.float32)
    terms = np.sign((q - dtarget.cpu().numpy()).astype(np.float32)).astype(np.float64) * (q.astype(np.float64) / float(dm))
    count = int((hd == np.float32(dscal[0])).sum())
    assert count >= 1
    want1 = -(w_depth * g_scale / (SW * SH)) * terms.sum() / count
    scale1 = (w_depth * g_scale / (SW * SH)) * np.abs(terms).sum() / count
    print(f"{SW}x{SH} depth loss: {d['tiles']} tiles, loss error {err:.2e}, max depth {dscal[0]:.6f} vs {M:.6f}, "
          f"max's gradient {dscal[1]:.4e} vs {want1:.4e}")
    assert err <= 1e-5
    assert abs(float(dscal[1]) - want1) <= 1e-5 * scale1
    assert all(bool(torch.isfinite(x).all()) for x in grads)


# ---- e. every word, under uneven load, with the hand-off buffers' contents changing -----------------------------------
LW, LH = 200, 120  # 8 views: ~3,000 work items of 64 pairs in one grid at 16-pixel tiles, ~1,900 at 32
LAUNCHES = 24


class Load:
    """Two more streams rendering something unrelated (512 x 512, 100,000 Gaussians: binning, forward and backward) with
    no synchronisation against the stream under test.  ``report`` says, from event times, how much of the launches under
    test ran while one of them was busy: a figure for the record, not an assertion (it depends on the host's pace)."""

    def __init__(self, env):
        self.env, dev = env, env.dev
        S = 512
        sc = orc.synthetic_scene(100_000, seed=8)
        self.t = [torch.from_numpy(a).to(dev).contiguous() for a in sc.arrays()]
        view, proj = orc.orbit_cameras(4, S, S)[2]
        self.gv = env.tr.make_view(view, proj, S, S, None, depth_grad=True)
        self.prep = env.tr.prepare_native(*self.t, self.gv)
        self.prep.plan()
        g = torch.Generator(device=dev).manual_seed(50)
        self.g = (torch.randn((S, S, 3), generator=g, device=dev), torch.randn((S, S), generator=g, device=dev),
                  torch.randn((S, S), generator=g, device=dev))
        torch.cuda.synchronize()
        self.streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
        self.pushed = 0
        self.spans, self.marks = [], []
        self.base = self.mark()

    @staticmethod
    def _event(stream=None):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(stream) if stream is not None else ev.record()
        return ev

    def mark(self):
        """An event on the stream under test (the current one)."""
        return self._event()

    def launch(self, fn):
        """fn() enqueues one launch under test; its span on the current stream is kept for the report."""
        a = self.mark()
        fn()
        self.marks.append((a, self.mark()))

    def push(self, times=1):
        tr = self.env.tr
        for st in self.streams:
            with torch.cuda.stream(st):
                a = self._event(st)
                for _ in range(times):
                    _, _, _, rs = tr.forward_native(*self.t, self.gv, prepared=self.prep)
                    tr.backward_native(*self.t, rs, *self.g)
                self.spans.append((a, self._event(st)))
        self.pushed += times

    def report(self) -> str:
        """Waits for everything, then: the launches under test that overlapped the other streams' work, and the share of
        their time that did."""
        torch.cuda.synchronize()
        busy = sorted((self.base.elapsed_time(a), self.base.elapsed_time(b)) for a, b in self.spans)
        merged = []
        for a, b in busy:
            if merged and a <= merged[-1][1]:
                merged[-1][1] = max(merged[-1][1], b)
            else:
                merged.append([a, b])
        hit, total, covered = 0, 0.0, 0.0
        for a, b in self.marks:
            t0, t1 = self.base.elapsed_time(a), self.base.elapsed_time(b)
            c = sum(max(0.0, min(t1, y) - max(t0, x)) for x, y in merged)
            hit += c > 0.0
            total += t1 - t0
            covered += c
        return (f"{self.pushed} unrelated renders on each of 2 other streams; {hit} of {len(self.marks)} launches overlapped "
                f"them, {100.0 * covered / max(total, 1e-9):.0f} % of the launches' {total:.2f} ms")


_IDLE: dict = {}


def _idle_expectation(env, tile):
    """Per colour set (A: the scene's, B: a second random set) and view: (loss, sums, out, alpha) of the single-view
    calls on an idle device, checked against the oracle as in (c); computed once per tile size."""
    if tile in _IDLE:
        return _IDLE[tile]
    tr, dev = env.tr, env.dev
    m, s, c, o = env.t
    cb = torch.from_numpy(env.colors_b).to(dev)
    HW = LW * LH
    exp = {"targets": [_target(env, LW, LH, 60 + k) for k in range(8)], "plans": [], "sets": {}}
    w_sil, g_scale = 0.2, 0.125
    for name, cc, ocol in (("A", c, None), ("B", cb, env.colors_b)):
        rows = []
        for k in range(8):
            target, mask = exp["targets"][k]
            gv = _gv(env, _cam(LW, LH, k, 8), LW, LH, ONE_ZONE, tile=tile, chunk=64)
            prep = tr.prepare_native(m, s, cc, o, gv)
            loss = torch.zeros(1, device=dev)
            out, alpha = torch.empty((LH, LW, 3), device=dev), torch.empty((LH, LW), device=dev)
            st, ws = tr.forward_l1_native(m, s, cc, o, gv, prep, target, mask, w_sil, g_scale, loss, out=out, alpha=alpha)
            tr.backward_splat_native(st, ws)
            sums = tr.gather_view_native(st, ws)
            torch.cuda.synchronize()
            if name == "A":
                exp["plans"].append(st.plan)
            o_out, o_alpha, _, ranges = _oracle_fwd(env, (k, 8), LW, LH, ONE_ZONE, tile, ocol)
            h_out, h_alpha = out.cpu().numpy().astype(np.float64), alpha.cpu().numpy().astype(np.float64)
            tn, mn = target.cpu().numpy(), mask.cpu().numpy()
            o_loss = np.abs(o_out.astype(np.float64) - tn).mean() + w_sil * np.abs(o_alpha.astype(np.float64) - mn).mean()
            errs = {"out": orc.rel_l2(h_out, o_out), "alpha": orc.rel_l2(h_alpha, o_alpha),
                    "loss": abs(float(loss) - o_loss) / o_loss}
            if k == 2:  # the gradients on the view of (c) (the oracle's backward is the slow part)
                grads = tuple(torch.empty_like(x) for x in (m, s, cc, o))
                tr.reduce_sums_native(m, s, cc, o, [(st.gv, sums)], grads, accumulate=False)
                g_rgb = (np.sign(h_out - tn) * (g_scale / (3 * HW))).astype(np.float32)
                g_a = (np.sign(h_alpha - mn) * (w_sil * g_scale / HW)).astype(np.float32)
                errs.update(_grad_errs(grads, _oracle_bwd(env, (k, 8), LW, LH, ONE_ZONE, tile, g_rgb, g_a, None, ocol), True))
            hr.assert_uneven(ranges, False)
            _assert_bars(f"idle {name} view {k} tile {tile}", errs,
                         _per_tile(h_out, h_alpha, o_out, o_alpha, ranges, 64, tile, LW, LH))
            rows.append((loss, sums, out, alpha))
        exp["sets"][name] = rows
    for k in range(8):  # the colour sets change every partial sum
        assert not torch.equal(exp["sets"]["A"][k][1], exp["sets"]["B"][k][1])
        assert not torch.equal(exp["sets"]["A"][k][2], exp["sets"]["B"][k][2])
    _IDLE[tile] = exp
    return exp


def _where(env, b, got, want, kind):
    """View-local description of the first mismatching word: its index, and the tile it belongs to with that tile's
    number of work items (for per-Gaussian sums: the Gaussian's heaviest tile)."""
    g, w = got.reshape(-1).cpu().numpy().view(np.uint32), want.reshape(-1).cpu().numpy().view(np.uint32)
    bad = np.nonzero(g != w)[0]
    d = _lists(env, b)
    items = hr.tile_items(d["ranges"], d["ch"])
    te, _ = _tiles(b.gv)
    tx = (b.gv.width + te - 1) // te
    word = int(bad[0])
    if kind == "loss":
        return f"{len(bad)} words differ, first word {word} (the view loss: every tile, {int(items.sum())} items)"
    if kind == "sums":
        gauss = word // 8
        K = int(hr.list_lengths(d["ranges"]).sum())
        cap = int(b.plan.num_pairs)
        ids = b.bins.cpu().numpy()[env.nat.bins_layout(b.gv, env.n, cap)[1]:][:4 * cap].view(np.int32)
        mine = [v // 2 for v, (a, e) in enumerate(d["ranges"]) if e > a and gauss in ids[a:e]]
        tile = max(mine, key=lambda t: items[t]) if mine else -1
        return (f"{len(bad)} words differ, first word {word} (Gaussian {gauss}, column {word % 8}; of its {len(mine)} tiles "
                f"tile {tile} has the most items: {int(items[tile]) if mine else 0}; {K} pairs)")
    per = 3 if kind == "out" else 1
    p = word // per
    tile = (p // b.gv.width // te) * tx + (p % b.gv.width) // te
    return (f"{len(bad)} words differ, first word {word} (pixel {p % b.gv.width},{p // b.gv.width}: tile {tile}, "
            f"{int(items[tile])} items)")


@pytest.mark.parametrize("sized", [False, True], ids=["host_sized", "device_sized"])
@pytest.mark.parametrize("tile", [16, 32])
def test_every_word_under_load(env, tile, sized):
    """24 launches (a fixed count) of preparation + gr_fit_views_batched on eight views at 64-pair items, alternating
    the colour sets A and B through the same geom / bins / scratch / ws, and after each one single-view
    gr_fwd_render_l1 with images through one view's same buffers; the results of every launch are kept and compared
    word for word with the idle device's afterwards (no host wait inside the loop)."""
    dev, nat, L, n = env.dev, env.nat, env.L, env.n
    exp = _idle_expectation(env, tile)
    m, s, c, o = env.t
    colors = {"A": c, "B": torch.from_numpy(env.colors_b).to(dev)}
    w_sil, g_scale = 0.2, 0.125
    bufs, gvs = [], []
    for k in range(8):
        gv = _gv(env, _cam(LW, LH, k, 8), LW, LH, ONE_ZONE, tile=tile, chunk=64)
        plan = exp["plans"][k]
        plan = nat.GrPlan(plan.num_pairs, max(plan.num_slots, plan.num_pairs), plan.num_core_pairs)
        if sized:
            gv = nat.GrView.from_buffer_copy(gv)
            gv.device_counts = 1
            plan = _caps(nat, plan)
        gvs.append(gv)
        bufs.append(Bufs(env, gv, plan))
    views = (nat.GrView * 8)(*gvs)
    gptr = (ctypes.c_void_p * 8)(*[b.geom.data_ptr() for b in bufs])
    plan_hosts = torch.zeros((8, 3), dtype=torch.int64, pin_memory=True)
    hptr = (ctypes.c_void_p * 8)(*[plan_hosts[k].data_ptr() for k in range(8)])
    capa = (nat.GrPlan * 8)(*[b.plan for b in bufs])
    overflow = torch.zeros(1, dtype=torch.int32, device=dev)
    nan = float("nan")
    r_loss = torch.full((LAUNCHES, 8), nan, device=dev)
    r_sums = torch.full((LAUNCHES, 8, n, 8), nan, device=dev)
    r_loss1 = torch.full((LAUNCHES,), nan, device=dev)
    r_out = torch.full((LAUNCHES, LH, LW, 3), nan, device=dev)
    r_alpha = torch.full((LAUNCHES, LH, LW), nan, device=dev)
    load = Load(env)
    torch.cuda.synchronize()
    load.push(4)
    for i in range(LAUNCHES):
        cc = colors["AB"[i % 2]]
        load.push()
        a_mark = load.mark()
        if sized:
            nat.check(L.gr_fwd_prepare_views_sized(8, views, n, nat.ptr(m), nat.ptr(s), nat.ptr(cc), 3, nat.ptr(o), gptr,
                                                   bufs[0].geom.numel(), capa, hptr, nat.ptr(overflow), env.stream()),
                      "gr_fwd_prepare_views_sized")
        else:
            nat.check(L.gr_fwd_prepare_views_async(8, views, n, nat.ptr(m), nat.ptr(s), nat.ptr(cc), 3, nat.ptr(o), gptr,
                                                   bufs[0].geom.numel(), hptr, env.stream()), "gr_fwd_prepare_views_async")
        arr = (nat.GrBatchView * 8)()
        for k, b in enumerate(bufs):
            target, mask = exp["targets"][k]
            _batch_entry(env, arr[k], b, target, mask, r_sums[i, k], r_loss[i, k:k + 1])
        _batched(env, arr, w_sil, 0.0, g_scale)
        k = i % 8
        target, mask = exp["targets"][k]
        _fwd_l1(env, bufs[k], target, mask, w_sil, g_scale, r_loss1[i:i + 1], out=r_out[i], alpha=r_alpha[i])
        load.marks.append((a_mark, load.mark()))
    busy = load.report()
    assert int(overflow) == 0
    for k in range(8):
        assert plan_hosts[k].tolist()[0] == exp["plans"][k].num_pairs
    total_items = sum(int(_lists(env, b)["num"][0]) for b in bufs)
    assert total_items >= 1800, total_items
    words = bad = 0
    first = None
    for i in range(LAUNCHES):
        rows = exp["sets"]["AB"[i % 2]]
        pairs = [(k, "loss", r_loss[i, k:k + 1], rows[k][0]) for k in range(8)]
        pairs += [(k, "sums", r_sums[i, k], rows[k][1]) for k in range(8)]
        k = i % 8
        pairs += [(k, "loss", r_loss1[i:i + 1], rows[k][0]), (k, "out", r_out[i], rows[k][2]),
                  (k, "alpha", r_alpha[i], rows[k][3])]
        for k, kind, got, want in pairs:
            words += got.numel()
            if not torch.equal(got, want):
                diff = int((got.reshape(-1).view(torch.int32) != want.reshape(-1).view(torch.int32)).sum())
                bad += diff
                if first is None:
                    first = f"launch {i} (set {'AB'[i % 2]}), view {k}, {kind}: " + _where(env, bufs[k], got, want, kind)
    print(f"under load, tile {tile}, {'device' if sized else 'host'}-sized: {LAUNCHES} launches, {total_items} work items per "
          f"grid, {words} words compared, {bad} mismatches; {busy}")
    assert bad == 0, first
    # the report of a mismatch, exercised on words that do differ (the two colour sets' expectations; alpha does not
    # depend on the colours: another view's)
    for kind, col in (("loss", 0), ("sums", 1), ("out", 2), ("alpha", 3)):
        other = exp["sets"]["B"][2][col] if kind != "alpha" else exp["sets"]["A"][3][col]
        text = _where(env, bufs[2], exp["sets"]["A"][2][col], other, kind)
        assert "words differ, first word" in text and ("items" in text), text
    for k, b in enumerate(bufs):
        _zero_tickets(env, b, f"the launches under load, view {k}")


def test_fit_activations_regulariser_under_load(env):
    """k_fit_activations' regulariser (1,024 blocks, arrive_last on one counter): two parameter sets alternating through
    one workspace under the same load, bit-equal to the idle device's each time; the counter is left zero."""
    dev, nat, L = env.dev, env.nat, env.L
    n = 100_000  # 3 n / 256 > 1,024: the full grid
    g = torch.Generator(device=dev).manual_seed(70)
    sets = [(torch.randn((n, 3), generator=g, device=dev) * sc, torch.randn((n,), generator=g, device=dev) * sc,
             torch.randn((n, 3), generator=g, device=dev)) for sc in (1.0, 3.0)]
    ws = torch.zeros((int(L.gr_fit_activations_ws_bytes(n)),), dtype=torch.uint8, device=dev)
    scales, opac, cols = torch.empty((n, 3), device=dev), torch.empty((n,), device=dev), torch.empty((n, 3), device=dev)
    w_s, w_o = 0.01, 0.02

    def run(p, reg):
        nat.check(L.gr_fit_activations(n, nat.ptr(p[0]), nat.ptr(p[1]), nat.ptr(p[2]), 3 * n, nat.ptr(scales), nat.ptr(opac),
                                       nat.ptr(cols), ctypes.c_float(w_s), ctypes.c_float(w_o), nat.ptr(reg), nat.ptr(ws),
                                       ws.numel(), env.stream()), "gr_fit_activations")

    idle = []
    for p in sets:
        reg = torch.full((1,), float("nan"), device=dev)
        run(p, reg)
        torch.cuda.synchronize()
        want = (np.float32(w_o) * np.float32(opac.double().mean().item())
                + np.float32(w_s) * np.float32(scales.double().mean().item()))
        assert abs(float(reg) - float(want)) <= 1e-6 * abs(float(want)), (float(reg), float(want))
        idle.append(reg)
    assert not torch.equal(idle[0], idle[1])
    load = Load(env)
    torch.cuda.synchronize()
    load.push(4)
    got = torch.full((LAUNCHES,), float("nan"), device=dev)
    for i in range(LAUNCHES):
        load.push()
        load.launch(lambda: run(sets[i % 2], got[i:i + 1]))
    busy = load.report()
    bad = [i for i in range(LAUNCHES) if not torch.equal(got[i:i + 1], idle[i % 2])]
    print(f"regulariser under load: {LAUNCHES} launches, {len(bad)} mismatches; {busy}")
    assert not bad, (bad, got.tolist(), [float(x) for x in idle])
    assert not ws[2 * 1024 * 8:].any()  # the arrival counter behind the 1,024 blocks' partial sums
