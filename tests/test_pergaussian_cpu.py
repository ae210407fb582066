"""CPU: the per-Gaussian gradient reference (tests/pergaussian_reference.py) and its checker.

a. The reference is right: its projection records equal the oracle's bit for bit, its images equal the float64 binned
   oracle's per pixel and its gradients equal the oracle's row by row and component by component within
   ``2^-21 a[i, k]`` (the oracle returns float32: at most 2^-24 |g| <= 2^-24 a of rounding, three bits over), on the
   three footprints the HIP tests use (the fit's one zone at 16- and 32-pixel tiles, the two-zone depth footprint), for
   colour dims 3, 12 and 48, with and without a depth gradient; its dense form equals oracle.dense_grads_sel.
b. The checker sees what the aggregate relL2 at 1e-4 does not: four defective copies of g made by the reference itself
   are all rejected at tau = 2^-16, three of them while their aggregate relL2 stays within 1e-4.

The scene's condition (every class with three members at both tile sizes, every live class with a member of two or more
kept tiles) is asserted here; the seed was picked for it.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import pergaussian_reference as pr
from conftest import load_pkg
from oracle import oracle as orc

W, H = pr.W_MIXED, pr.H_MIXED
BG = (0.2, 0.5, 0.7)
REF_BAR = 2.0 ** -21


def _footprints():
    tr = load_pkg().torch_renderer
    return {"fit16": (tr.FIT_CUTOFF, tr.FIT_CUTOFF, 16), "fit32": (tr.FIT_CUTOFF, tr.FIT_CUTOFF, 32),
            "depth": (tr.DEPTH_GRAD_CUTOFF, tr.DEFAULT_CORE_CUTOFF, 16)}


@functools.lru_cache(maxsize=None)
def _scene(cd: int) -> orc.Scene:
    sc = pr.mixed_scene()
    return sc if cd == 3 else pr.sh_colors(sc, cd // 3)


@functools.lru_cache(maxsize=None)
def _fp(name: str) -> pr.Footprint:
    cutoff, core, tile = _footprints()[name]
    return pr.footprint(_scene(3), pr.camera(), W, H, cutoff, core, tile)


@functools.lru_cache(maxsize=4)
def _forward(name: str, cd: int) -> pr.Forward:
    return pr.forward(_scene(cd), pr.camera(), W, H, _fp(name), BG)


def _oview(name, background=BG):
    cutoff, core, tile = _footprints()[name]
    cam = pr.camera()
    return orc.make_view(cam[0], cam[1], W, H, background, cutoff=cutoff, core_cutoff=core, tile=tile)


def _upstreams(seed=5):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((H, W, 3)).astype(np.float32), rng.standard_normal((H, W)).astype(np.float32),
            rng.standard_normal((H, W)).astype(np.float32))


def _classes(name):
    return pr.classes(_scene(3), pr.camera(), W, H, _fp(name), _footprints()[name][0])


# ---- the scene ------------------------------------------------------------------------------------------------------
def test_scene_shape_and_classes():
    sc = _scene(3)
    assert sc.means.shape == (601, 3) and 601 % 64 and 601 % 256
    assert W % 16 and H % 16 and W % 32 and H % 32  # ragged at both tile sizes in both axes
    for name in ("fit16", "fit32", "depth"):
        fp, cl = _fp(name), _classes(name)
        multi = fp.kept.sum(1) >= 2
        for c in pr.CLASSES:
            assert int(cl[c].sum()) >= 3, (name, c, int(cl[c].sum()))
        for c in pr.LIVE_CLASSES:
            assert (cl[c] & multi).any(), (name, c)
        assert int(cl["zero_opacity"].sum()) >= 2
    assert _fp("depth").tail.any() and not _fp("fit16").tail.any()
    # the SH variants: part of the rows' evaluated colours leave [0, 1] (the clamp masks their colour gradient), not all
    for cd in (12, 48):
        s2 = _scene(cd)
        col = pr.eval_colors(s2.colors, s2.means, orc.camera_position(pr.camera()[0]))
        outside = ((col < 0) | (col > 1)).any(1)
        assert 10 <= int(outside.sum()) <= 300, (cd, int(outside.sum()))


@pytest.mark.parametrize("cd", [3, 12, 48])
def test_projection_records_equal_the_oracles(cd):
    """Computed here on their own, compared bit for bit: centre, sigma, depth, validity, clamped colour."""
    sc = _scene(cd)
    cam = pr.camera()
    rec, _, _ = orc.preprocess(_oview("fit16"), sc)
    p = pr.project(sc.means, sc.scales, cam[0], cam[1], W, H)
    for j, a in ((0, p.px), (1, p.py), (2, p.sx), (3, p.sy), (8, p.za)):
        np.testing.assert_array_equal(rec[:, j], a)
    np.testing.assert_array_equal(rec[:, 11] != 0, p.valid)
    col = pr.eval_colors(sc.colors, sc.means, orc.camera_position(cam[0]))
    np.testing.assert_array_equal(rec[:, 5:8], np.clip(col, 0, 1))


# ---- a. the reference against the oracle ----------------------------------------------------------------------------
@pytest.mark.parametrize("cd", [3, 12, 48])
@pytest.mark.parametrize("name", ["fit16", "fit32", "depth"])
def test_reference_equals_oracle_row_by_row(name, cd):
    fw = _forward(name, cd)
    v = _oview(name)
    o_out, o_alpha, o_depth = orc.forward(v, fw.scene, binned=True)
    # float32 images of float64 sums: half an ulp each, 2^-21 leaves three bits (out relative to its own scale of 1)
    assert np.abs(fw.out - o_out).max() <= REF_BAR
    assert (np.abs(fw.alpha - o_alpha) <= REF_BAR * fw.alpha).all()
    assert (np.abs(fw.depth - o_depth) <= REF_BAR * fw.depth).all()
    g_rgb, g_a, g_d = _upstreams()
    cl = _classes(name)
    for depth in (None, g_d):
        g, a = pr.backward(fw, g_rgb, g_a, depth)
        ora = orc.backward(v, fw.scene, g_rgb, g_a, depth, binned=True)
        for k, o in zip(pr.NAMES, ora):
            assert (a[k] * (1 + 1e-12) >= np.abs(g[k])).all(), k
            r = pr.assert_rows(o, g[k], a[k], REF_BAR, cl, fw.fp, f"{name} cd {cd} depth {depth is not None} {k}")
            assert pr.zero_components_exact(o, a[k]), k
            print(f"{name} cd {cd} depth {depth is not None} {k}: worst |oracle - g| / a = {r:.2e}")
        assert (a["d_scales"][:, 2] == 0).all() and (a["d_means"][cl["dead"]] == 0).all()


def test_dense_form_equals_dense_grads_sel():
    """The dead rows and 20 others over the whole image (no footprint) with the binned forward's per-pixel sums, on a
    12-sigma one-zone footprint: tiles beyond it hold weights below exp(-72) of the peak, so the dense rows also equal
    the binned ones within the bar."""
    sc, cam = _scene(3), pr.camera()
    fp = pr.footprint(sc, cam, W, H, 12.0, 12.0, 16)
    fw = pr.forward(sc, cam, W, H, fp, BG)
    cl = pr.classes(sc, cam, W, H, fp, 12.0)
    dead = np.nonzero(~(fw.p.valid & (sc.opacities >= 0)))[0]
    assert len(dead) >= 3
    rng = np.random.default_rng(9)
    others = rng.choice(np.nonzero(fp.kept.any(1))[0], 20, replace=False)
    sel = np.concatenate([dead, others]).astype(np.int32)
    g_rgb, g_a, g_d = _upstreams(6)
    v = orc.make_view(cam[0], cam[1], W, H, BG, cutoff=12.0, core_cutoff=12.0)
    for depth in (None, g_d):
        gd, ad = pr.backward(fw, g_rgb, g_a, depth, dense=True)
        gb, ab = pr.backward(fw, g_rgb, g_a, depth)
        ora = orc.dense_grads_sel(v, sc, sel, g_rgb, g_a, depth)
        for k, o in zip(pr.NAMES, ora):
            pr.assert_rows(o, gd[k][sel], ad[k][sel], REF_BAR, {c: m[sel] for c, m in cl.items()}, None, f"dense {k}")
            pr.assert_rows(o, gb[k][sel], ab[k][sel], REF_BAR, {c: m[sel] for c, m in cl.items()}, None, f"binned {k}")
            assert (o[:len(dead)] == 0).all()


# ---- b. the checker -------------------------------------------------------------------------------------------------
def _rejected(defect, g, a, cl, fp):
    """The arrays of the defective copy the checker rejects at tau = 2^-16."""
    bad = []
    for k in pr.NAMES:
        try:
            pr.assert_rows(defect[k], g[k], a[k], pr.TAU, cl, fp, k)
        except AssertionError as e:
            bad.append(k)
            print(str(e)[:300])
    return bad


def _aggregate(defect, g):
    return max(orc.rel_l2(defect[k], g[k]) for k in pr.NAMES)


def test_checker_rejects_what_the_aggregate_passes():
    name = "fit16"
    fw, fp, cl = _forward(name, 3), _fp(name), _classes(name)
    g_rgb, g_a, _ = _upstreams(7)
    g, a = pr.backward(fw, g_rgb, g_a, None)
    for k in pr.NAMES:  # the reference itself passes, as does its float32 rounding
        assert pr.assert_rows(g[k].astype(np.float32), g[k], a[k], 2.0 ** -23, cl, fp, k) <= 2.0 ** -24

    # (i) one ragged Gaussian's terms in one of its tiles left out.  Candidates in ascending gradient norm (the rows the
    # aggregate weighs least); the first whose defect the aggregate passes is taken.
    norms = np.sqrt(sum((g[k].reshape(len(g[k]), -1) ** 2).sum(1) for k in pr.NAMES))
    last = np.nonzero((np.arange(fp.kept.shape[1]) % fp.tiles_x == fp.tiles_x - 1)
                      | (np.arange(fp.kept.shape[1]) // fp.tiles_x == fp.tiles_y - 1))[0]
    cand = [i for i in np.argsort(norms) if cl["ragged"][i] and fp.kept[i].sum() >= 2 and norms[i] > 0]
    found = None
    for i in cand[len(cand) // 2:][:4]:  # from the median-norm ragged row on
        t = int(last[np.nonzero(fp.kept[i, last])[0][0]])
        gi, _ = pr.backward(fw, g_rgb, g_a, None, drop=(int(i), t))
        if _aggregate(gi, g) <= 1e-4 and len(_rejected(gi, g, a, cl, fp)) > 0:
            found = (int(i), t, _aggregate(gi, g))
            break
    assert found is not None, "no ragged Gaussian whose dropped tile the aggregate passes and the checker rejects"
    print(f"(i) Gaussian {found[0]} without its tile {found[1]}: aggregate relL2 {found[2]:.2e}")

    # (ii) the weak class x 1.005 in the arrays that scale with the opacity (d_opac = sum gw E does not: a weak row's is
    # as large as any other's, and the aggregate does see it)
    d2 = {k: g[k].copy() for k in pr.NAMES}
    for k in ("d_means", "d_scales", "d_colors"):
        d2[k][cl["weak"]] *= 1.005
    assert _aggregate(d2, g) <= 1e-4
    assert _rejected(d2, g, a, cl, fp) == ["d_means", "d_scales", "d_colors"]

    # (iii) one anisotropic Gaussian's d_scales columns 0 and 1 swapped
    i3 = int(np.nonzero(cl["anisotropic"] & (a["d_scales"][:, 0] > 0) & (a["d_scales"][:, 1] > 0))[0][0])
    d3 = {k: g[k].copy() for k in pr.NAMES}
    d3["d_scales"][i3, [0, 1]] = d3["d_scales"][i3, [1, 0]]
    assert _rejected(d3, g, a, cl, fp) == ["d_scales"]

    # (iv) one dead row 1e-9 instead of 0
    i4 = int(np.nonzero(cl["dead"])[0][0])
    d4 = {k: g[k].copy() for k in pr.NAMES}
    d4["d_means"][i4] = 1e-9
    assert _aggregate(d4, g) <= 1e-4
    assert _rejected(d4, g, a, cl, fp) == ["d_means"]
    assert not pr.zero_components_exact(d4["d_means"], a["d_means"])
