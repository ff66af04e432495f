"""CPU tests of the mosaic layer (include/meteor_demod_amd_mosaic.h): the host model of the blend against the numpy restatement of
mosaic_util.py on hand-made node grids, one pass against the map layer's model, the order of the passes, answers that need no model,
the common grid against the map layer's and against the numpy inverse of map_ref.py, a scene of latitude / longitude squares seen by
two passes through the whole CPU path, the joint stretch, the binding, and the C host without a mosaic layer.  Every test prints
the figures it asserts on."""
from __future__ import annotations

import functools
import re
import subprocess

import numpy as np
import pytest

import map_util as MU
import mosaic_util as Z
import picture_util as PU
import test_map_host as H
from conftest import ROOT
from test_gpu_map import SELECTS

MODES = (Z.FEATHER, Z.BEST)
COUNTS = (1, 2, 3, 8)


# ------------------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("kind", ["mixed", "empty1"])
def test_model_blend_equals_the_numpy_reference(kind):
    """Sizes 4 x 1, 36 x 150 and 200 x 150; 1, 2, 3 and 8 passes of 3 and 5 strip rows, among them nodes of any int32 and a pass with
    all nodes missing; both modes; every selection: bytes, valid and cover."""
    from meteor_demod_amd import mosaic as M
    for w, h in Z.SIZES:
        for n in COUNTS:
            bad, overlap = 0, 0
            for select in SELECTS:
                src = Z.sources(kind, w, h, n, len(select))
                for mode in MODES:
                    got = M.model_blend(src, select, w, h, mode, valid=True, cover=True)
                    want = Z.blend_reference(src, select, w, h, mode)
                    bad += sum(int((a != b).sum()) for a, b in zip(got, want))
                    assert np.array_equal(M.model_blend(src, select, w, h, mode), want[0])         # valid = cover = NULL
                    overlap = max(overlap, int(((want[2] & (want[2] - 1)) != 0).sum()))
            print(f"{kind}, {w} x {h}, {n} passes: {bad} bytes differ; up to {overlap} pixels seen by two or more passes")
            assert bad == 0 and (n == 1 or overlap >= 4) and (n == 1 or w < 200 or overlap > 0.3 * w * h)       # (the passes do overlap)
            if n >= 3:
                assert not (want[2] & 4).any()                                                     # the pass with all nodes missing


def test_one_pass_is_the_map_layers_warp():
    from meteor_demod_amd import map as MP, mosaic as M
    for kind in ("mixed", "empty1"):
        images, filled, luts = H._source(kind)
        for name, w, h, nodes in MU.warp_cases():
            for select in ((2, 1, 0), (1,), (0, 0, 2)):
                want, want_val = MP.model_warp(images, filled, select, luts[: len(select)], nodes, w, h, valid=True)
                for mode in MODES:
                    out, val, cov = M.model_blend([(images, filled, luts[: len(select)], nodes)], select, w, h, mode, valid=True, cover=True)
                    assert np.array_equal(out, want) and np.array_equal(val, want_val) and np.array_equal(cov, (want_val != 0).astype(np.uint8)), (kind, name, select, mode)


def test_order_of_the_passes():
    """FEATHER is a sum: a permutation of the passes leaves pixels and valid alone and permutes the bits of cover.  BEST takes the
    lower pass of two that weigh the same: of two identical passes only pass 0's bit is set."""
    from meteor_demod_amd import mosaic as M
    w, h, select = 200, 150, (2, 1, 0)
    src = Z.sources("mixed", w, h, 3, 3)
    out, val, cov = M.model_blend(src, select, w, h, Z.FEATHER, valid=True, cover=True)
    for perm in ((1, 0, 2), (2, 0, 1), (2, 1, 0)):
        o2, v2, c2 = M.model_blend([src[k] for k in perm], select, w, h, Z.FEATHER, valid=True, cover=True)
        back = np.zeros_like(c2)
        for at, k in enumerate(perm):
            back |= ((c2 >> at) & 1) << k
        assert np.array_equal(o2, out) and np.array_equal(v2, val) and np.array_equal(back, cov), perm
    o1, v1, c1 = M.model_blend(src[:1], select, w, h, Z.BEST, valid=True, cover=True)
    o2, v2, c2 = M.model_blend([src[0], src[0]], select, w, h, Z.BEST, valid=True, cover=True)
    print(f"{int((c2 == 1).sum())} pixels of pass 0, {int((c2 > 1).sum())} of pass 1")
    assert np.array_equal(o2, o1) and np.array_equal(v2, v1) and np.array_equal(c2, c1) and set(np.unique(c2)) == {0, 1}
    # FEATHER of two identical passes is the pass itself: (2 w b + w) / 2 w = b
    of, vf, cf = M.model_blend([src[0], src[0]], select, w, h, Z.FEATHER, valid=True, cover=True)
    assert np.array_equal(of, o1) and np.array_equal(vf, v1) and np.array_equal(cf, 3 * c1)


def test_known_answers():
    """Weights that can be read off the nodes: pass A at the left edge of its swath (w = 1 + j), pass B at nadir (w = 784 - j)."""
    from meteor_demod_amd import mosaic as M
    ident = np.arange(256, dtype=np.uint8)[None]

    def const(rows, level):
        return [np.full((8 * rows, 1568), level, np.uint8)] * 3, [np.ones((rows, 14), np.uint8)] * 3
    a_nodes = MU.affine_nodes(4, 1, lambda i, j: 256 * j, lambda i, j: 256 * 10 + 0 * i)
    b_nodes = MU.affine_nodes(4, 1, lambda i, j: 256 * (783 + j) + 128, lambda i, j: 256 * 800 + 0 * i)
    for la, lb in ((0, 255), (255, 0), (100, 200)):
        a, b = (*const(3, la), ident, a_nodes), (*const(200, lb), ident, b_nodes)
        out, cov = M.model_blend([a, b], (0,), 4, 1, Z.FEATHER, cover=True)
        want = [((1 + j) * la + (784 - j) * lb + (785 >> 1)) // 785 for j in range(4)]
        print(f"levels {la} and {lb}: {out[0, :, 0].tolist()}, expected {want}")
        assert out[0, :, 0].tolist() == want and (cov == 3).all()
        assert (M.model_blend([a, b], (0,), 4, 1, Z.BEST)[0, :, 0] == lb).all() and (M.model_blend([b, a], (0,), 4, 1, Z.BEST)[0, :, 0] == lb).all()
    assert ((784 * 255 + 392) // 785, (1 * 255 + 392) // 785) == (255, 0)
    # equal weights: the mean, halves rounded up
    a, b = (*const(3, 10), ident, a_nodes), (*const(3, 21), ident, a_nodes)
    assert (M.model_blend([a, b], (0,), 4, 1, Z.FEATHER)[0, :, 0] == 16).all() and (M.model_blend([a, b], (0,), 4, 1, Z.BEST)[0, :, 0] == 10).all()
    # an empty pass (None: rows = 0) counts nowhere
    out, cov = M.model_blend([None, b], (0,), 4, 1, Z.FEATHER, cover=True)
    assert (out == 21).all() and (cov == 2).all()


# ------------------------------------------------------------------------------------------------------------------ grid
B_RAAN, B_LATER = 158.0, 20


def _pass_b_text():
    return MU.with_raan(B_RAAN)


def _plain_pass(rows, s0, text):
    from meteor_demod_amd import mosaic as M
    place, info = MU.packets(rows, s0)
    return M.Pass(text, [np.zeros((8 * rows, 1568), np.uint8), None, None], [np.ones((rows, 14), np.uint8), None, None], place, info)


def test_grid_of_one_pass_is_the_map_layers():
    from meteor_demod_amd import map as MP, mosaic as M
    rows = 120
    p = _plain_pass(rows, MU.mid_latitude_s0(), MU.tle_text())
    for opts in (dict(px_per_deg=40), dict(px_per_deg=25, side=-1, scan_deg=100)):
        g = M.grid([p], **opts)
        want = MP.grid(MU.tle_text(), MP.fit_time(p.place, p.sinfo), 8 * rows, **opts)
        print(f"{g.width} x {g.height} at {g.sx} x {g.sy:g} from {g.lat_top}, {g.lon_left}")
        assert (g.width, g.height, g.sx, g.sy, g.lat_top, g.lon_left) == (want.width, want.height, want.sx, want.sy, want.lat_top, want.lon_left)
        assert g.nodes.shape == (1, *want.nodes.shape) and np.array_equal(g.nodes[0], want.nodes)
        assert (g.passes[0].date, g.passes[0].lines, g.passes[0].rows_fit) == (want.date, 8 * rows, rows)


def test_grid_of_two_passes():
    """Every node of both passes against the numpy model's own inverse, to the tolerance of test_map_host: 1 unit of 1/256 pixel.
    The union holds both single grids."""
    from meteor_demod_amd import mosaic as M
    rows_a, rows_b = 120, 88
    s0 = MU.mid_latitude_s0()
    a, b = _plain_pass(rows_a, s0, MU.tle_text()), _plain_pass(rows_b, s0 + B_LATER * MU.ROW_PERIOD, _pass_b_text())
    g = M.grid([a, b], px_per_deg=40)
    refs = (MU.ref_pass(rows_a), MU.ref_pass(rows_b, s0=s0 + B_LATER * MU.ROW_PERIOD, text=_pass_b_text()))
    ia, ib = np.meshgrid(16 * np.arange(g.nodes.shape[1]), 16 * np.arange(g.nodes.shape[2]), indexing="ij")
    lat, lon = g.lat_top - (ia + 0.5) / g.sy, g.lon_left + (ib + 0.5) / g.sx
    for k, (ref, rows) in enumerate(zip(refs, (rows_a, rows_b))):
        y, x = ref.inverse(lat, lon, lines=8 * rows)
        n = g.nodes[k]
        none = (n[..., 0] == MU.NO_NODE) & (n[..., 1] == MU.NO_NODE)
        both = ~none & np.isfinite(y)
        ex, ey = np.abs(n[..., 0][both] - 256 * x[both]), np.abs(n[..., 1][both] - 256 * y[both])
        print(f"pass {k}: {int(none.sum())} of {none.size} nodes missing ({int(np.isnan(y).sum())} in numpy); worst difference {ex.max():.3f} in X, {ey.max():.3f} in Y")
        assert np.array_equal(none, np.isnan(y)) and 0 < none.sum() < none.size and ex.max() <= 1.0 and ey.max() <= 1.0
        assert g.passes[k].lines == 8 * rows and g.passes[k].date == 19822
    assert g.width % 4 == 0 and g.nodes.shape[1:] == MU.nodes_shape(g.width, g.height)
    for p in (a, b):
        one = M.grid([p], px_per_deg=40)
        top, left = (g.lat_top - one.lat_top) * g.sy, ((one.lon_left - g.lon_left + 180) % 360 - 180) * g.sx
        bottom, right = top + one.height, left + one.width * g.sx / one.sx
        print(f"single grid {one.width} x {one.height} inside {g.width} x {g.height}: lines {top:.1f} .. {bottom:.1f}, columns {left:.1f} .. {right:.1f}")
        assert top >= -1e-6 and left >= -1.0 and bottom <= g.height + 1e-6 and right <= g.width + 1.0     # (sx differs: a pixel of rounding)
    # the order decides the reference longitude only: the same box to a pixel
    swapped = M.grid([b, a], px_per_deg=40)
    assert abs(swapped.width - g.width) <= 4 and swapped.height == g.height and (swapped.sx, swapped.lat_top) == (g.sx, g.lat_top)


def test_grid_refusals():
    from meteor_demod_amd import _capi, mosaic as M
    rows, s0 = 120, MU.mid_latitude_s0()
    a = _plain_pass(rows, s0, MU.tle_text())
    far = _plain_pass(rows, s0, MU.with_raan(150.0 + 120.0))
    polar = _plain_pass(600, MU.mid_latitude_s0(50.0), MU.tle_text())
    for word, fn in (("no pass", lambda: M.grid([])), ("1 .. 8", lambda: M.grid([a] * 9)), ("beyond 85", lambda: M.grid([a, polar], px_per_deg=20)),
                     ("fits", lambda: M.grid([a, far], px_per_deg=100)), ("1 .. 1000", lambda: M.grid([a], px_per_deg=1001)),
                     ("scan side", lambda: M.grid([a], side=0)), ("stretch", lambda: M.grid([a], stretch=3)), ("blend", lambda: M.grid([a], blend=2)),
                     ("piece_lines", lambda: M.grid([a], piece_lines=24)), ("no element set", lambda: M.grid([_plain_pass(rows, s0, "hello\n")])),
                     ("catalogue number 5", lambda: M.grid([M.Pass(a.tle_text, a.images, a.filled, a.place, a.sinfo, norad=5)])),
                     ("no placed packet", lambda: M.grid([M.Pass(a.tle_text, a.images, a.filled, a.place[:0], a.sinfo[:0])]))):
        with pytest.raises(_capi.MdemodError) as e:
            fn()
        print(f"{word}: '{e.value.detail}'")
        assert e.value.code == _capi.MDEMOD_ERR_PARAM and word in e.value.detail
    with pytest.raises(_capi.MdemodError) as e:
        M.grid([a, far], px_per_deg=100)
    fit = int(re.search(r"scale of (\d+) fits", e.value.detail).group(1))
    ok = M.grid([a, far], px_per_deg=fit)
    print(f"two passes 120 degrees apart at 100 px/deg refused, the scale named is {fit}: {ok.width} x {ok.height}")
    assert ok.width <= 8192 and ok.height <= 16384 and ok.width > 4096


# ------------------------------------------------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def e2e_passes():
    """Pass A: test_map_host.e2e_case() as it is.  Pass B: the same orbit with its node 8 degrees further east, 20 row periods later,
    painted from the same scene, with its own 10 % of strips lost.  (passes, marked square)."""
    from meteor_demod_amd import mosaic as M
    images, filled, place, info, ref, marked = H.e2e_case()
    rng = np.random.default_rng(22)
    s0 = MU.mid_latitude_s0() + B_LATER * MU.ROW_PERIOD
    ref_b = MU.ref_pass(H.E2E_ROWS, s0=s0, text=_pass_b_text())
    keep = rng.random((H.E2E_ROWS, 3, 14)) >= 0.1
    place_b, info_b = MU.packets(H.E2E_ROWS, s0, keep=keep)
    b = M.Pass(_pass_b_text(), MU.paint(ref_b, H.E2E_ROWS, H.SQUARE, marked), MU.filled_of(place_b, H.E2E_ROWS), place_b, info_b)
    return [M.Pass(MU.tle_text(), images, filled, place, info), b], marked


@functools.lru_cache(maxsize=None)
def e2e_model(mode, piece_lines=64):
    from meteor_demod_amd import mosaic as M
    passes, _ = e2e_passes()
    return M.model_host(passes, (2, 1, 0), stretch=0, px_per_deg=50, blend=mode, piece_lines=piece_lines)


@pytest.mark.parametrize("mode", MODES)
def test_two_pass_scene_through_the_cpu_model(mode):
    """check_scene holds only if both passes land on the common lattice where the ground is; the mosaic fills what one pass lost."""
    from meteor_demod_amd import mosaic as M
    passes, marked = e2e_passes()
    m = e2e_model(mode)
    print(f"{m.width} x {m.height}, {100 * m.valid_share:.1f} % valid, {100 * m.overlap_share:.1f} % seen by both, marked square at {marked}")
    H.check_scene(m, marked, f"model, blend {mode}")
    whole = e2e_model(mode, 16384)
    assert np.array_equal(whole.pixels, m.pixels) and np.array_equal(whole.valid, m.valid) and np.array_equal(whole.cover, m.cover)
    g = M.grid(passes, px_per_deg=50)
    assert (g.width, g.height, g.sx, g.sy, g.lat_top, g.lon_left) == (m.width, m.height, m.sx, m.sy, m.lat_top, m.lon_left)
    ident = np.arange(256, dtype=np.uint8)[None].repeat(3, 0)
    filled_where_a_is_black, alone = 0, []
    for k, p in enumerate(passes):
        out, val = M.model_blend([(p.images, p.filled, ident, g.nodes[k])], (2, 1, 0), g.width, g.height, mode, valid=True)
        assert not (val & ~m.valid).any()                                          # valid of the mosaic holds valid of each pass alone
        alone.append(val != 0)
        assert m.passes[k].covered == np.count_nonzero(m.cover & (1 << k)) and not ((m.cover >> k) & 1 & (val == 0)).any()
        assert mode == Z.BEST or m.passes[k].covered == np.count_nonzero(val)
        if k == 0:
            filled_where_a_is_black = int(((val == 0) & (m.valid == 7)).sum())
            inside_a = M.model_blend([(p.images, [np.ones_like(f) for f in p.filled], ident[:1], g.nodes[k])], (2,), g.width, g.height, mode, valid=True)[1] != 0
            holes = int((inside_a & (val != 7) & (m.valid == 7)).sum())
    both, only_a, only_b = [x.sum() / m.cover.size for x in (alone[0] & alone[1], alone[0] & ~alone[1], alone[1] & ~alone[0])]
    assert mode == Z.BEST or np.array_equal(m.cover, alone[0] + 2 * alone[1])
    print(f"seen by both {100 * both:.1f} %, by A alone {100 * only_a:.1f} %, by B alone {100 * only_b:.1f} %; {filled_where_a_is_black} pixels black in A alone and "
          f"filled in the mosaic, {holes} of them inside A's swath")
    assert both >= 0.20 and only_a >= 0.05 and only_b >= 0.05
    assert filled_where_a_is_black > 0 and holes > 0
    assert m.overlap_pixels == (m.cover == 3).sum() and m.valid_pixels == np.count_nonzero(m.valid) and (mode == Z.BEST or m.overlap_share == both)
    assert [r.date for r in m.passes] == [19822, 19822] and [r.rows_fit for r in m.passes] == [H.E2E_ROWS] * 2
    assert all(abs(r.row_period - MU.ROW_PERIOD) < 1e-9 and r.limits == [(0, 255)] * 3 for r in m.passes)
    assert abs(m.passes[1].utc0 - m.passes[0].utc0 - B_LATER * MU.ROW_PERIOD) < 1e-6
    wld = [float(v) for v in m.world_file().split()]
    assert wld == [1 / m.sx, 0, 0, -1 / m.sy, m.lon_left + 0.5 / m.sx, m.lat_top - 0.5 / m.sy]


# --------------------------------------------------------------------------------------------------------------- stretch
@functools.lru_cache(maxsize=None)
def stretch_passes():
    """Two short passes of random bytes of different brightness, with holes."""
    from meteor_demod_amd import mosaic as M
    rng = np.random.default_rng(31)
    out = []
    for k, (rows, text, later, top) in enumerate(((40, MU.tle_text(), 0, 256), (32, _pass_b_text(), 6, 140))):
        s0 = MU.mid_latitude_s0(40.0) + later * MU.ROW_PERIOD
        place, info = MU.packets(rows, s0, keep=rng.random((rows, 3, 14)) >= 0.15)
        images = [rng.integers(20 * k, top, (8 * rows, 1568), dtype=np.uint8) for _ in range(3)]
        out.append(M.Pass(text, images, MU.filled_of(place, rows), place, info))
    return out


def test_joint_stretch_is_the_picture_layers_rule_on_the_summed_histograms():
    from meteor_demod_amd import map as MP, mosaic as M
    passes = stretch_passes()
    hists = [PU.histogram(p.images, p.filled).astype(np.int64) for p in passes]
    for select, opts in (((2, 1, 0), dict(px_per_deg=30)), ((1,), dict(px_per_deg=30, clip_low=100, clip_high=20)), ((0, 0, 2), dict(px_per_deg=30, blend="best"))):
        clips = opts.get("clip_low", 5), opts.get("clip_high", 5)
        g = M.grid(passes, **opts)
        for stretch in (1, 2, 0):
            m = M.model_host(passes, select, stretch=stretch, **opts)
            if stretch == 1:
                tabs = [[PU.lut(hists[0][s] + hists[1][s], *clips) for s in select]] * 2
            elif stretch == 2:
                tabs = [[PU.lut(h[s], *clips) for s in select] for h in hists]
            else:
                tabs = [[(np.arange(256, dtype=np.uint8), 0, 255)] * len(select)] * 2
            src = [(p.images, p.filled, np.stack([t[0] for t in tabs[k]]), g.nodes[k]) for k, p in enumerate(passes)]
            want = M.model_blend(src, select, g.width, g.height, opts.get("blend", "feather"), valid=True, cover=True)
            px = m.pixels if len(select) == 3 else m.pixels[..., None]
            print(f"select {select}, stretch {stretch}: limits {[r.limits for r in m.passes]}, {100 * m.overlap_share:.1f} % seen by both")
            assert np.array_equal(px, want[0]) and np.array_equal(m.valid, want[1]) and np.array_equal(m.cover, want[2])
            assert [r.limits for r in m.passes] == [[(t[1], t[2]) for t in tabs[k]] for k in range(2)]
            assert "blend" in opts or m.overlap_share > 0.05                      # (with BEST two bits want two planes with different winners)
    # one pass: the map layer's result in every setting that has a counterpart there
    p = passes[0]
    for stretch in (0, 1, 2):
        one = M.model_host([p], (2, 1, 0), stretch=stretch, px_per_deg=30)
        want = MP.model_host(p.tle_text, p.images, p.filled, p.place, p.sinfo, (2, 1, 0), stretch=min(stretch, 1), px_per_deg=30)
        assert np.array_equal(one.pixels, want.pixels) and np.array_equal(one.valid, want.valid) and one.passes[0].limits == want.limits
        assert (one.sx, one.sy, one.lat_top, one.lon_left, one.passes[0].utc0, one.passes[0].date) == (want.sx, want.sy, want.lat_top, want.lon_left, want.utc0, want.date)


def test_compose_refusals_of_the_model():
    from meteor_demod_amd import _capi, mosaic as M
    passes = stretch_passes()
    for word, fn in (("no pass", lambda: M.model_host([], (0,))), ("1 .. 8", lambda: M.model_host([passes[0]] * 9, (0,))), ("planes", lambda: M.model_host(passes, (0, 1))),
                     ("slot", lambda: M.model_host(passes, (3,))), ("blend", lambda: M.model_host(passes, (0,), blend=2)),
                     ("slot 1 ", lambda: M.model_host([passes[0], M.Pass(passes[1].tle_text, [passes[1].images[0], None, None], [passes[1].filled[0], None, None],
                                                                             passes[1].place, passes[1].sinfo)], (1,)))):
        with pytest.raises(_capi.MdemodError) as e:
            fn()
        print(f"{word}: '{e.value.detail}'")
        assert e.value.code == _capi.MDEMOD_ERR_PARAM and word in e.value.detail


# ---------------------------------------------------------------------------------------------------------------- binding
def _header_entries():
    return re.findall(r"^\s*(?:int|void|uint64_t)\s+(mdemod_\w+)\s*\(", (ROOT / "include" / "meteor_demod_amd_mosaic.h").read_text(), re.M)


def test_mosaic_entries_exported_and_bound():
    from meteor_demod_amd import _capi, image, map as MP, mosaic as M, picture
    names = _header_entries()
    assert sorted(names) == sorted(["mdemod_mosaic_default_opts", "mdemod_mosaic_grid", "mdemod_mosaic_grid_free", "mdemod_mosaic_blend_device",
                                    "mdemod_mosaic_compose_host", "mdemod_mosaic_free"])
    lib = M.lib()
    for n in names + list(M.MODEL_SIGNATURES):
        assert hasattr(lib, n), n
    assert sorted(M.SIGNATURES) == sorted(names)
    assert sorted(M.MODEL_SIGNATURES) == ["mdemod_mosaic_model_blend", "mdemod_mosaic_model_host"]
    others = (list(_capi.SIGNATURES) + list(image.SIGNATURES) + list(image.MODEL_SIGNATURES) + list(picture.SIGNATURES) + list(picture.MODEL_SIGNATURES) +
              list(MP.SIGNATURES) + list(MP.MODEL_SIGNATURES))
    assert not any("mosaic" in n for n in others)
    text = (ROOT / "include" / "meteor_demod_amd_mosaic.h").read_text()
    assert "mdemod_map_" not in text
    for h in (ROOT / "include").glob("*.h"):
        if h.name != "meteor_demod_amd_mosaic.h":
            assert "mdemod_mosaic_" not in h.read_text(), h.name
    assert _capi.lib().mdemod_abi_version() == 5
    for f in ("make_opts", "grid", "blend", "compose", "images_to_mosaic", "model_blend", "model_host"):
        assert callable(getattr(M, f))
    o = M.make_opts()
    assert (o.scan_deg, o.px_per_deg, o.time_offset, o.row_period, o.side, o.stretch, o.clip_low, o.clip_high, o.piece_lines, o.blend) == \
           (110.0, 100.0, 10800.0, 8 / 6.5, 1, 1, 5, 5, 0, 0)
    assert M.make_opts(blend="best").blend == 1
    with pytest.raises(TypeError):
        M.make_opts(date=3)


def test_mosaic_int_entries_are_function_try_blocks():
    from meteor_demod_amd import mosaic as M
    found = 0
    entries = set(_header_entries()) | set(M.MODEL_SIGNATURES)
    for src in (ROOT / "meteor_demod_amd" / "csrc" / "mosaic.hip", ROOT / "meteor_demod_amd" / "csrc" / "mosaic_host.cpp"):
        text = src.read_text()
        for m in re.finditer(r"^int\n(mdemod_\w+)\(", text, re.M):
            assert m.group(1) in entries, m.group(1)
            found += 1
            body = text[m.end():]
            assert body[: body.index("{")].rstrip().endswith("try"), f"{src.name}: {m.group(1)} is not a function-try-block"
            assert body[body.index("{"):].lstrip("{ ").startswith("MDEMOD_API_ENTER"), m.group(1)
            assert body[body.index("\n}"):].startswith("\n} MDEMOD_API_CATCH"), f"{src.name}: {m.group(1)} does not end in MDEMOD_API_CATCH"
    assert found == 2 + 3, found
    listed = (ROOT / "meteor_demod_amd" / "csrc" / "mosaic_host.h").read_text()
    assert all(n in listed for n in M.MODEL_SIGNATURES)


def test_mosaic_struct_layouts(tmp_path):
    import ctypes as C
    from meteor_demod_amd import mosaic as M
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "meteor_demod_amd_mosaic.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", '
           'sizeof(mdemod_mosaic_opts), sizeof(mdemod_mosaic_pass), sizeof(mdemod_mosaic_timing), sizeof(mdemod_mosaic_nodes), sizeof(mdemod_mosaic_source), '
           'sizeof(mdemod_mosaic_result), offsetof(mdemod_mosaic_opts, blend), offsetof(mdemod_mosaic_pass, n_desc), offsetof(mdemod_mosaic_pass, rows), '
           'offsetof(mdemod_mosaic_timing, lines), offsetof(mdemod_mosaic_nodes, nodes), offsetof(mdemod_mosaic_source, rows), offsetof(mdemod_mosaic_result, utc0), '
           'offsetof(mdemod_mosaic_result, covered), offsetof(mdemod_mosaic_result, cover)); return 0;}')
    (tmp_path / "s.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")], check=True)
    out = [int(x) for x in subprocess.run([str(tmp_path / "s")], capture_output=True, text=True, check=True).stdout.split()]
    print(out)
    assert out == [C.sizeof(M.MdemodMosaicOpts), C.sizeof(M.MdemodMosaicPass), C.sizeof(M.MdemodMosaicTiming), C.sizeof(M.MdemodMosaicNodes),
                   C.sizeof(M.MdemodMosaicSource), C.sizeof(M.MdemodMosaicResult), M.MdemodMosaicOpts.blend.offset, M.MdemodMosaicPass.n_desc.offset,
                   M.MdemodMosaicPass.rows.offset, M.MdemodMosaicTiming.lines.offset, M.MdemodMosaicNodes.nodes.offset, M.MdemodMosaicSource.rows.offset,
                   M.MdemodMosaicResult.utc0.offset, M.MdemodMosaicResult.covered.offset, M.MdemodMosaicResult.cover.offset]
    assert C.sizeof(M.MdemodMosaicSource) == 72


# ------------------------------------------------------------------------------------------------- the C host, no mosaic
def test_cli_without_mosaic_layer_links_and_refuses(tmp_path):
    """The C host against tests/sanitize/stub_backend.c (which has no mosaic layer): it links, --help lists --mosaic and
    --mosaic-blend, and --mosaic exits with status 1 saying what the library lacks, and writes nothing.  Against the real library
    --mosaic without --map, a ninth file and an unknown blend are refused before anything is demodulated."""
    import frames_util as U
    exe = tmp_path / "cli_stub"
    r = subprocess.run(["gcc", "-std=gnu11", "-O1", "-Wall", "-I", str(ROOT / "include"), str(ROOT / "host" / "meteor_demod_amd.c"),
                        str(ROOT / "tests" / "sanitize" / "stub_backend.c"), "-pthread", "-lm", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    h = subprocess.run([str(exe), "--help"], capture_output=True, text=True)
    assert h.returncode == 0 and all(w in h.stderr for w in ("--mosaic <base>", "--mosaic-blend"))
    wav = tmp_path / "in.wav"
    wav.write_bytes(U.wav_bytes(288000, np.zeros((16384, 2), dtype=np.int16)))
    tle = MU.GOLDEN / "map_tle.txt"
    r = subprocess.run([str(exe), "-q", "-o", str(tmp_path / "out.s"), "--image", "--map", str(tle), "--mosaic", "all", str(wav)], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 1 and "no mosaic layer" in r.stderr and "unrecognized" not in r.stderr, r.stderr
    r = subprocess.run([str(exe), "-q", "-o", str(tmp_path / "out.s"), "--image", "--mosaic", "all", str(wav)], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 1 and "no mosaic layer" in r.stderr and "unrecognized" not in r.stderr, r.stderr
    assert r.stdout == "" and sorted(p.name for p in tmp_path.iterdir()) == ["cli_stub", "in.wav"]
    cli_exe = ROOT / "meteor_demod_amd" / "lib" / "meteor_demod_amd"
    nine = [str(wav)] * 9
    for flags, files, word in ((("--image", "--mosaic", "all"), [str(wav)], "only with --map"), (("--mosaic", "all"), [str(wav)], "only with --map"),
                               (("--image", "--map", str(tle), "--mosaic-blend", "best"), [str(wav)], "only with --mosaic"),
                               (("--image", "--map", str(tle), "--mosaic", "all", "--mosaic-blend", "median"), [str(wav)], "feather or best"),
                               (("--image", "--map", str(tle), "--mosaic", "all"), nine, "1 .. 8")):
        r = subprocess.run([str(cli_exe), "-q", "-B", *flags, *files], capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == 1 and word in r.stderr and r.stdout == "", (flags, r.stderr)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["cli_stub", "in.wav"]
