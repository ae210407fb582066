"""GPU: every Gaussian's gradient error bounded, not just the aggregate norm.

Each HIP entry point that forms gradients runs once on tests/pergaussian_reference.py's mixed scene (601 Gaussians at
104 x 72: ragged at both tile sizes in both axes; sub-pixel, huge, anisotropic, weak, straddling, on-boundary, dead,
zero-opacity and negative-scale rows; colours over [0, 1], SH colours that leave it) against the term-wise float64
reference of the same operation:

* images per pixel: ``|hip - ref| <= tau_img * m + phi`` with m = ref for alpha and depth and ref_out + ref_alpha for
  out (the accumulators are sums of non-negative terms);
* the loss scalar, where the entry has one, within what the image bars allow the mean of 1-Lipschitz terms to move
  plus 2^-20 of float32 summation;
* gradients: ``|hip - g[i, k]| <= tau * a[i, k]`` for every Gaussian and component (pergaussian_reference.assert_rows;
  no absolute floor), a the sum of the absolute values of g's terms;
* every component with a == 0 (dead rows, the colour-clamped and sigma-clamped components, d_scales[:, 2]) exactly 0.0
  after a sentinel pre-fill, or after a zero fill with accumulate != 0.

The cap of every bar is 2^-16, include/gr_hip.h's contract for no_depth_grad = 1 views (the other modes are
f32-grade); the bars committed in BARS are min(2^-16, 4 x the worst measured on an MI355X) rounded up to one digit,
per family and array (profiles/per_gaussian_bars.txt has the measurements and the class of each worst row).

Families: 1. gr_fwd_render (k_raster_fwd_mfma<1> / <2> / <3>) with gr_bwd / gr_bwd_indexed, random upstreams, non-zero
background; 2. the fit path at 16-pixel tiles (gr_fwd_render_l1 with no_depth_grad 1 and 2, gr_bwd_splat,
gr_gather_view + gr_reduce_sums and gr_reduce_views); 3. the same at 32-pixel tiles (k_fwd32_l1 / k_bwd32); 4. gr_bwd_fit
with a depth target.  The L1 families' reference upstream takes the HIP images' signs (as test_tile32_gpu.py), so no
pixel is excluded at the kink.
"""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

import pergaussian_reference as pr
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

W, H = pr.W_MIXED, pr.H_MIXED
HW = W * H
BG = (0.2, 0.5, 0.7)
TAU = pr.TAU
SENTINEL = 7.5
W_SIL, W_DEPTH, G_SCALE = 0.2, 0.1, 0.25
IMG_SMALL = 2.0 ** -16  # below this multiplier a pixel is judged by phi alone when phi is measured

# Bars per family: images (tau_img, phi), gradients tau.  min(2^-16, 4 x measured worst) rounded up to one digit; phi
# is 4 x the worst |hip - ref| over pixels whose multiplier is below 2^-16 and at most 2^-16 x the image's maximum.
BARS = {
    # f32-grade W and D (three bf16 pieces), colours in two pieces: the images' colour part and d_colors are 2^-16 grade
    "render_mfma1": {"out": (TAU, 0.0), "alpha": (2e-6, 0.0), "depth": (2e-6, 0.0),
                     "d_means": 4e-6, "d_scales": 2e-6, "d_colors": TAU, "d_opac": 4e-6},
    # no_depth_grad = 1 with the depth output: W and D in two bf16 pieces too.  alpha's 7e-5 is 4 x its measured worst,
    # which is over the cap: one term's product is within 1.25 x 2^-16 and a pixel that one Gaussian reaches has one
    # term
    "render_mfma2": {"out": (TAU, 0.0), "alpha": (7e-5, 0.0), "depth": (TAU, 0.0),
                     "d_means": 7e-6, "d_scales": 1e-5, "d_colors": TAU, "d_opac": 8e-6},
    "render_mfma3": {"out": (7e-7, 0.0), "alpha": (4e-6, 0.0),
                     "d_means": 7e-6, "d_scales": 7e-6, "d_colors": TAU, "d_opac": 8e-6},
    # the fit forwards' f16 operands leave an absolute floor where only weak far tails reach
    "fit16": {"out": (2e-6, 1e-8), "alpha": (3e-6, 1e-8),
              "d_means": 1e-5, "d_scales": TAU, "d_colors": TAU, "d_opac": TAU},
    "fit16_f32": {"out": (TAU, 0.0), "alpha": (3e-6, 0.0),
                  "d_means": 2e-6, "d_scales": 2e-6, "d_colors": 2e-6, "d_opac": 4e-6},
    "fit32": {"out": (1e-6, 2e-8), "alpha": (2e-6, 2e-8),
              "d_means": 5e-6, "d_scales": TAU, "d_colors": TAU, "d_opac": TAU},
    "bwd_fit_depth": {"out": (TAU, 0.0), "alpha": (2e-6, 0.0), "depth": (2e-6, 0.0),
                      "d_means": 6e-6, "d_scales": 6e-6, "d_colors": TAU, "d_opac": 8e-6},
}


# ---- shared state ---------------------------------------------------------------------------------------------------
class Env:
    def __init__(self, pkg, dev):
        self.tr, self.nat, self.dev = pkg.torch_renderer, pkg._native, dev
        tr = self.tr
        self.cam = pr.camera()
        self.footprints = {"fit16": (tr.FIT_CUTOFF, tr.FIT_CUTOFF, 16), "fit32": (tr.FIT_CUTOFF, tr.FIT_CUTOFF, 32),
                           "depth": (tr.DEPTH_GRAD_CUTOFF, tr.DEFAULT_CORE_CUTOFF, 16),
                           "nodepth": (tr.DEFAULT_CUTOFF, tr.DEFAULT_CORE_CUTOFF, 16)}
        self._scenes, self._fp, self._fw, self._cl, self._t = {}, {}, {}, {}, {}
        rng = np.random.default_rng(31)
        self.g_rgb = rng.standard_normal((H, W, 3)).astype(np.float32)
        self.g_a = rng.standard_normal((H, W)).astype(np.float32)
        self.g_d = rng.standard_normal((H, W)).astype(np.float32)
        g = torch.Generator(device=dev).manual_seed(12)
        self.target = torch.rand((H, W, 3), generator=g, device=dev)
        self.mask = (self.target.mean(dim=2) > 0.5).float().contiguous()
        self.dtarget = torch.rand((H, W), generator=g, device=dev)

    def scene(self, cd=3, n=None) -> orc.Scene:
        """The mixed scene with colour dim cd; n = 65: its first 65 rows, n = 1: its one largest Gaussian."""
        key = (cd, n)
        if key not in self._scenes:
            sc = pr.mixed_scene()
            sc = sc if cd == 3 else pr.sh_colors(sc, cd // 3)
            if n == 1:
                sc = pr.one_huge(sc)
            elif n is not None:
                sc = pr.head(sc, n)
            self._scenes[key] = sc
        return self._scenes[key]

    def tensors(self, cd=3, n=None):
        key = (cd, n)
        if key not in self._t:
            self._t[key] = [torch.from_numpy(a).to(self.dev).contiguous() for a in self.scene(cd, n).arrays()]
        return self._t[key]

    def fp(self, name, n=None) -> pr.Footprint:
        if (name, n) not in self._fp:
            cutoff, core, tile = self.footprints[name]
            self._fp[(name, n)] = pr.footprint(self.scene(3, n), self.cam, W, H, cutoff, core, tile)
        return self._fp[(name, n)]

    def classes(self, name, n=None):
        if (name, n) not in self._cl:
            self._cl[(name, n)] = pr.classes(self.scene(3, n), self.cam, W, H, self.fp(name, n), self.footprints[name][0])
        return self._cl[(name, n)]

    def forward(self, name, cd, bg, n=None) -> pr.Forward:
        """The reference's forward, built once per footprint, colour dim and background and left unchanged."""
        key = (name, cd, bg, n)
        if key not in self._fw:
            self._fw[key] = pr.forward(self.scene(cd, n), self.cam, W, H, self.fp(name, n), bg)
        return self._fw[key]

    def view(self, name, bg=None, ndg=1, chunk=0):
        cutoff, core, tile = self.footprints[name]
        gv = self.tr.make_view(self.cam[0], self.cam[1], W, H, bg, cutoff=cutoff, core_cutoff=core, depth_grad=ndg == 0,
                               tile=tile if tile == 32 else 0)
        gv.no_depth_grad = ndg
        gv.chunk = chunk
        return gv

    def grads(self, t, fill):
        return tuple(torch.full_like(x, fill) for x in t)


@pytest.fixture(scope="module")
def env(pkg, cuda):
    return Env(pkg, cuda)


# ---- checks ---------------------------------------------------------------------------------------------------------
def _image(tag, name, hip, ref, mult, bar):
    """Print the image's figures (the worst |hip - ref| over the pixels with m < 2^-16, which phi is four times; the
    worst (|hip - ref| - phi) / m, which tau_img is four times or the cap), then assert |hip - ref| <= tau_img * m + phi
    everywhere."""
    tau_img, phi = bar
    hip, ref, mult = (np.asarray(x, np.float64) for x in (hip, ref, mult))
    assert hip.shape == ref.shape == mult.shape and np.isfinite(hip).all(), (tag, name)
    err = np.abs(hip - ref)
    small = mult < IMG_SMALL
    floor = float(err[small].max()) if small.any() else 0.0
    pos = mult > 0.0
    rel = np.where(pos, np.maximum(err - phi, 0.0) / np.where(pos, mult, 1.0), 0.0)
    at = np.unravel_index(int(np.argmax(rel)), rel.shape)
    print(f"PERGAUSSIAN {tag} {name}: ratio {float(rel[at]):.3e} beyond phi {phi:.1e} at pixel (y, x[, c]) {tuple(int(i) for i in at)}; "
          f"floor {floor:.3e} over the {int(small.sum())} pixels below 2^-16; image max {ref.max():.3e}")
    assert phi <= IMG_SMALL * ref.max()
    bad = err > tau_img * mult + phi
    if bad.any():
        p = np.unravel_index(int(np.argmax(np.where(bad, err - tau_img * mult - phi, -np.inf))), err.shape)
        raise AssertionError(f"{tag} {name}: pixel {p}: hip {hip[p]!r}, reference {ref[p]!r}, |error| {err[p]:.3e} > "
                             f"{tau_img:.3e} * {mult[p]:.3e} + {phi:.3e}; {int(bad.sum())} such pixels")
    return tau_img * mult + phi


def _images(tag, bars, fw, out, alpha, depth=None):
    """out, alpha (and depth) per pixel; returns the per-pixel bounds that held (the loss's bar builds on them)."""
    bounds = {"out": _image(tag, "out", out, fw.out, fw.out + fw.alpha[..., None], bars["out"]),
              "alpha": _image(tag, "alpha", alpha, fw.alpha, fw.alpha, bars["alpha"])}
    if depth is not None:
        bounds["depth"] = _image(tag, "depth", depth, fw.depth, fw.depth, bars["depth"])
    return bounds


def _gradients(tag, bars, hip, g, a, cl, fp):
    """assert_rows on the four arrays and the exact zeros; prints each array's worst ratio and its row's classes."""
    for k, h in zip(pr.NAMES, hip):
        h = h.cpu().numpy()
        ratio, i, comp, cls, _ = pr.worst_row(h, g[k], a[k], cl, fp)
        zeros = int((a[k] == 0).sum())
        print(f"PERGAUSSIAN {tag} {k}: ratio {ratio:.3e} Gaussian {i} component {comp} classes {','.join(cls)} "
              f"(zero components {zeros})")
        bad = (a[k] == 0) & (h != 0)
        assert not bad.any(), (tag, k, "components with a == 0 that are not exactly 0.0", np.argwhere(bad)[:5].tolist(),
                               h[bad][:5].tolist())
        pr.assert_rows(h, g[k], a[k], bars[k], cl, fp, f"{tag} {k}")
    assert (a["d_scales"][:, 2] == 0).all() and (a["d_means"][cl["dead"]] == 0).all()


def _np(x):
    return x.cpu().numpy().astype(np.float64)


def _l1_upstream(h_out, h_alpha, tn, mn):
    """The L1 loss's upstream from the HIP images' signs (near-ties depend on the last float bit)."""
    g_rgb = np.sign(h_out - tn) * (G_SCALE / (3 * HW))
    g_a = np.sign(h_alpha - mn) * (W_SIL * G_SCALE / HW)
    return g_rgb, g_a


def _loss(tag, hip_loss, want, allowed):
    print(f"PERGAUSSIAN {tag} loss: |hip - ref| {abs(hip_loss - want):.3e} of {want:.6f}, allowed {allowed:.3e}")
    assert math.isfinite(hip_loss) and abs(hip_loss - want) <= allowed, (tag, hip_loss, want, allowed)


# ---- 1. the render op -----------------------------------------------------------------------------------------------
def _render_op(env, mode, cd, indexed=False):
    tr, nat, dev = env.tr, env.nat, env.dev
    ndg = 0 if mode == "mfma1" else 1
    want_depth = mode != "mfma3"
    name = "depth" if ndg == 0 else "nodepth"
    bars = BARS["render_" + mode]
    tag = f"render_{mode} cd={cd}" + (" indexed" if indexed else "")
    t = env.tensors(cd)
    n = int(t[0].shape[0])
    rendered, index = t, None
    if indexed:  # the render is of a permuted copy; parameters and gradients stay in the caller's order
        q = np.random.default_rng(3).permutation(n)
        inv = np.empty(n, np.int32)
        inv[q] = np.arange(n, dtype=np.int32)
        qt = torch.from_numpy(q).to(dev)
        rendered = [x[qt].contiguous() for x in t]
        index = torch.from_numpy(inv).to(dev)
    gv = env.view(name, BG, ndg)
    out, alpha, depth, st = tr.forward_native(*rendered, gv, want_depth=want_depth)
    assert (depth is not None) == want_depth
    g_d = env.g_d if ndg == 0 else None
    up = [torch.from_numpy(x).to(dev) if x is not None else None for x in (env.g_rgb, env.g_a, g_d)]
    grads = env.grads(t, SENTINEL)
    tr._backward_call("gr_bwd_indexed" if indexed else "gr_bwd", st, dev, [nat.ptr(x) for x in up], t, grads, index=index)
    torch.cuda.synchronize()
    fw = env.forward(name, cd, BG)
    _images(tag, bars, fw, _np(out), _np(alpha), _np(depth) if want_depth else None)
    g, a = pr.backward(fw, env.g_rgb, env.g_a, g_d)
    _gradients(tag, bars, grads, g, a, env.classes(name), fw.fp)


@pytest.mark.parametrize("cd", [3, 48])
@pytest.mark.parametrize("mode", ["mfma1", "mfma2", "mfma3"])
def test_render_op(env, mode, cd):
    """gr_fwd_render in its three modes (f32-grade with a depth gradient on the two-zone 8-sigma view; no_depth_grad = 1
    with and without the depth output) and gr_bwd with random normal upstreams, background (0.2, 0.5, 0.7)."""
    _render_op(env, mode, cd)


def test_render_op_indexed(env):
    """gr_bwd_indexed: the render of a randomly permuted copy, the gradients back in the caller's order."""
    _render_op(env, "mfma1", 3, indexed=True)


# ---- 2. and 3. the fit path -----------------------------------------------------------------------------------------
def _fit_path(env, name, ndg, cd, chunk, n=None):
    tr, dev = env.tr, env.dev
    family = "fit32" if name == "fit32" else ("fit16_f32" if ndg == 2 else "fit16")
    bars = BARS[family]
    tag = f"{family} cd={cd} chunk={chunk}" + (f" n={n}" if n else "")
    t = env.tensors(cd, n)
    gv = env.view(name, None, ndg, chunk)
    prep = tr.prepare_native(*t, gv)
    loss = torch.full((1,), SENTINEL, device=dev)
    out, alpha = torch.full((H, W, 3), SENTINEL, device=dev), torch.full((H, W), SENTINEL, device=dev)
    st, ws = tr.forward_l1_native(*t, gv, prep, env.target, env.mask, W_SIL, G_SCALE, loss, out=out, alpha=alpha)
    tr.backward_splat_native(st, ws)
    sums = tr.gather_view_native(st, ws)
    by_sums = env.grads(t, SENTINEL)
    tr.reduce_sums_native(*t, [(st.gv, sums)], by_sums, accumulate=False)
    by_views = env.grads(t, 0.0)
    tr.reduce_views_native(*t, [(st, ws)], by_views, accumulate=True)
    torch.cuda.synchronize()
    fw = env.forward(name, cd, None, n)
    h_out, h_alpha = _np(out), _np(alpha)
    bounds = _images(tag, bars, fw, h_out, h_alpha)
    tn, mn = _np(env.target), _np(env.mask)
    want = np.abs(fw.out - tn).mean() + W_SIL * np.abs(fw.alpha - mn).mean()
    _loss(tag, float(loss), want, bounds["out"].mean() + W_SIL * bounds["alpha"].mean() + 2.0 ** -20 * want)
    g_rgb, g_a = _l1_upstream(h_out, h_alpha, tn, mn)
    g, a = pr.backward(fw, g_rgb, g_a, None)
    cl = env.classes(name, n)
    _gradients(tag + " reduce_sums", bars, by_sums, g, a, cl, fw.fp)
    _gradients(tag + " reduce_views", bars, by_views, g, a, cl, fw.fp)


@pytest.mark.parametrize("chunk", [64, 0])
@pytest.mark.parametrize("cd", [3, 12])
@pytest.mark.parametrize("ndg", [1, 2])
def test_fit_path_tile16(env, ndg, cd, chunk):
    """k_raster_fwd_mfma<4> (no_depth_grad = 1) / <5> (= 2, f32 grade), the 16-pixel backward splat, k_gather_view +
    k_reduce_sums (written over a sentinel) and k_reduce_views (accumulated into zeros)."""
    _fit_path(env, "fit16", ndg, cd, chunk)


@pytest.mark.parametrize("cd,chunk", [(3, 64), (3, 0), (48, 0)])
def test_fit_path_tile32(env, cd, chunk):
    """k_fwd32_l1 / k_bwd32 through the same calls."""
    _fit_path(env, "fit32", 1, cd, chunk)


@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("name", ["fit16", "fit32"])
def test_fit_path_few_gaussians(env, name, n):
    """One huge Gaussian alone, and the first 65 rows (one more than a wave, a quarter of a block)."""
    _fit_path(env, name, 1, 3, 0, n)


# ---- 4. gr_bwd_fit with a depth target ------------------------------------------------------------------------------
def test_bwd_fit_depth(env):
    """gr_fwd_render (f32-grade, two zones, cutoff 8) + gr_bwd_fit with w_depth = 0.1: the loss
    mean|out - t| + w_sil mean|alpha - m| + w_depth mean|depth / (max depth + 1e-6) - t_d| and its gradients, written
    over a sentinel and accumulated into zeros."""
    tr, dev = env.tr, env.dev
    bars, tag = BARS["bwd_fit_depth"], "bwd_fit_depth"
    t = env.tensors(3)
    gv = env.view("depth", None, 0)
    out, alpha, depth, st = tr.forward_native(*t, gv, want_depth=True)
    loss = torch.full((1,), SENTINEL, device=dev)
    written, added = env.grads(t, SENTINEL), env.grads(t, 0.0)
    tr.backward_fit_native(*t, st, env.target, env.mask, W_SIL, env.dtarget, W_DEPTH, G_SCALE, loss, written, False)
    tr.backward_fit_native(*t, st, env.target, env.mask, W_SIL, env.dtarget, W_DEPTH, G_SCALE, loss, added, True)
    torch.cuda.synchronize()
    fw = env.forward("depth", 3, None)
    h_out, h_alpha, h_depth = _np(out), _np(alpha), _np(depth)
    bounds = _images(tag, bars, fw, h_out, h_alpha, h_depth)
    tn, mn, dt = _np(env.target), _np(env.mask), _np(env.dtarget)
    M = fw.depth.max()
    dm = M + 1e-6
    q = fw.depth / dm
    want = np.abs(fw.out - tn).mean() + W_SIL * np.abs(fw.alpha - mn).mean() + W_DEPTH * np.abs(q - dt).mean()
    # |d (d / (M + 1e-6))| <= (|dd| + q |dM|) / (M + 1e-6) to first order; twice that covers the second
    dq = 2.0 * (bounds["depth"] + q * bounds["depth"].max()) / dm
    _loss(tag, float(loss), want,
          bounds["out"].mean() + W_SIL * bounds["alpha"].mean() + W_DEPTH * dq.mean() + 2.0 ** -20 * want)
    # upstream: signs and the arg-max pixel from the HIP images, magnitudes from the reference
    g_rgb, g_a = _l1_upstream(h_out, h_alpha, tn, mn)
    hd32 = depth.cpu().numpy()
    hm = np.float32(hd32.max())
    top = hd32 == hm
    assert int(top.sum()) == 1 and fw.depth[top][0] == M  # one arg-max pixel, the reference's
    sgn = np.sign((hd32 / (hm + np.float32(1e-6))).astype(np.float32) - env.dtarget.cpu().numpy()).astype(np.float64)
    c = W_DEPTH * G_SCALE / HW
    g_d = sgn * c / dm
    a_d = np.abs(g_d)
    g_d[top] += -c * (sgn * q / dm).sum()
    a_d[top] += c * (np.abs(sgn) * q / dm).sum()
    g, a = pr.backward(fw, g_rgb, g_a, g_d, a_depth=a_d)
    cl = env.classes("depth")
    _gradients(tag + " written", bars, written, g, a, cl, fw.fp)
    _gradients(tag + " accumulated", bars, added, g, a, cl, fw.fp)
