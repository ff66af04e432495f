"""CPU tests of the polar layer (include/meteor_demod_amd_polar.h): the projection against a published value, its own inverse and the
numpy model of polar_ref.py; the frame of passes over the top and the bottom of the orbit with its refusals; the host nodes against
the numpy model's own inverse in projected coordinates, the pole among them; what the 16-pixel grid costs on such a pass; a scene of
latitude / longitude squares through the whole CPU path, alone and with a second pass; vertices and graticule; the binding.  Every
test prints the figures it asserts on."""
from __future__ import annotations

import functools
import re
import subprocess

import numpy as np
import pytest

import map_util as MU
import polar_ref as PR
import polar_util as PU_
from conftest import ROOT


# ------------------------------------------------------------------------------------------------------------ projection
def test_published_value():
    """EPSG guidance note 7-2, polar stereographic variant B: lat_ts 71 S, lon0 70 E, the point 75 S 120 E; easting 7 255 380.79 and
    northing 7 053 389.56 with false origins of 6 000 000."""
    from meteor_demod_amd import polar as P
    e, n = P.forward(-1, 71.0, 70.0, -75.0, 120.0)
    re_, rn = PR.Proj(-1, 71.0, 70.0).forward(-75.0, 120.0)
    print(f"C: E {float(e):.3f}, N {float(n):.3f}; numpy: E {float(re_):.3f}, N {float(rn):.3f}")
    for got in ((e, n), (re_, rn)):
        assert abs(got[0] - 1255380.79) <= 0.01 and abs(got[1] - 1053389.56) <= 0.01
    lat, lon = P.inverse(-1, 71.0, 70.0, e, n)
    assert abs(lat + 75.0) < 1e-9 and abs(lon - 120.0) < 1e-9


@pytest.mark.parametrize("pole", [1, -1])
def test_projection_round_trip_mirror_and_reference(pole):
    from meteor_demod_amd import polar as P
    rng = np.random.default_rng(5 + pole)
    lat_ts, lon0 = 70.0, 33.0
    lat = pole * np.concatenate([rng.uniform(0.5, 90.0, 9990), [90.0, 90.0, 89.999999, 45.0, 45.0, 10.0, 60.0, 60.0, 1.0, 89.0]])
    lon = np.concatenate([rng.uniform(-180.0, 180.0, 9990), [0.0, lon0, lon0, lon0 + 180.0, lon0 - 180.0, lon0 + 180.0, -180.0, 179.999999, lon0, lon0 - 180.0]])
    e, n = P.forward(pole, lat_ts, lon0, lat, lon)
    la, lo = P.inverse(pole, lat_ts, lon0, e, n)
    at_pole = np.abs(lat) == 90.0
    d_lat, d_lon = np.abs(la - lat).max(), np.abs((lo - lon + 180.0) % 360.0 - 180.0)[~at_pole].max()
    print(f"pole {pole}: forward then inverse off by {d_lat:.2e} degrees of latitude, {d_lon:.2e} of longitude; the pole comes back at longitude {lo[at_pole].tolist()}")
    assert d_lat <= 1e-9 and d_lon <= 1e-9 and (lo[at_pole] == lon0).all() and (e[at_pole] == 0).all() and (n[at_pole] == 0).all()
    # the other pole is this one mirrored: the same E, the opposite N
    e2, n2 = P.forward(-pole, lat_ts, lon0, -lat, lon)
    assert np.abs(e2 - e).max() <= 1e-6 and np.abs(n2 + n).max() <= 1e-6
    # the numpy model, both ways
    ref = PR.Proj(pole, lat_ts, lon0)
    re_, rn = ref.forward(lat, lon)
    rla, rlo = ref.inverse(e, n)
    d = max(np.abs(re_ - e).max(), np.abs(rn - n).max())
    print(f"C against numpy: {d:.2e} m forward, {np.abs(rla - la).max():.2e} degrees inverse")
    assert d <= 1e-6 and np.abs(rla - la).max() <= 1e-9 and np.abs((rlo - lo + 180.0) % 360.0 - 180.0)[~at_pole].max() <= 1e-9
    # a standard parallel at the pole itself is the limit of the formula
    e90, n90 = P.forward(pole, 90.0, lon0, lat, lon)
    e89, n89 = P.forward(pole, 89.9999, lon0, lat, lon)
    assert np.abs(e90 - e89).max() <= 1e-3 * max(1.0, np.abs(e90).max() / 1e6) and np.abs(n90 - n89).max() <= 1e-3 * max(1.0, np.abs(n90).max() / 1e6)


# ----------------------------------------------------------------------------------------------------------------- frame
@functools.lru_cache(maxsize=None)
def polar_grid(first_u=PU_.POLAR_U, rows=PU_.POLAR_ROWS, res=1000.0):
    from meteor_demod_amd import polar as P
    return P.grid([PU_.polar_pass(first_u, rows)[0]], metres_per_pixel=res)


def test_frame_of_a_pass_over_the_top():
    from meteor_demod_amd import _capi, map as MP, polar as P
    p, ref = PU_.polar_pass()
    lines = 8 * PU_.POLAR_ROWS
    with pytest.raises(_capi.MdemodError) as e:                                    # the latitude / longitude grid has no place for it
        MP.grid(MU.tle_text(), MP.fit_time(p.place, p.sinfo), lines)
    assert "beyond 85" in e.value.detail
    g = polar_grid()
    f = g.frame
    proj = PU_.proj_of(f)
    lat_c, lon_c = ref.forward((lines - 1) / 2, 783.5)
    print(f"{f.width} x {f.height} at {f.res:g} m from E {f.e_left:.0f}, N {f.n_top:.0f}; pole {f.pole}, lat_ts {f.lat_ts_deg}, lon0 {f.lon0_deg} (centre pixel at {lat_c:.3f}, {lon_c:.3f})")
    assert f.pole == 1 and f.lat_ts_deg == 70.0 and f.lon0_deg == np.floor(lon_c + 0.5) and f.width % 4 == 0 and g.nodes.shape[1:] == f.nodes_shape
    assert f.e_left % f.res == 0 and f.n_top % f.res == 0
    # the corners of the picture and the pole lie inside
    lat, lon = ref.forward(np.array([0.0, 0.0, lines - 1.0, lines - 1.0]), np.array([0.0, 1567.0, 0.0, 1567.0]))
    e_, n_ = proj.forward(np.append(lat, 90.0), np.append(lon, 0.0))
    j, i = (e_ - f.e_left) / f.res, (f.n_top - n_) / f.res
    print(f"corners and pole at columns {np.round(j, 1).tolist()}, lines {np.round(i, 1).tolist()}")
    assert (j >= 0).all() and (j <= f.width).all() and (i >= 0).all() and (i <= f.height).all()
    # no more than a pixel larger than the border's box (the width is rounded up to a multiple of 4 besides)
    ys = np.unique(np.append(np.arange(0, lines, 8), lines - 1)).astype(float)
    xs = np.unique(np.append(np.arange(0, 1568, 16), 1567)).astype(float)
    by, bx = np.concatenate([ys, ys, np.zeros_like(xs), np.full_like(xs, lines - 1)]), np.concatenate([np.zeros_like(ys), np.full_like(ys, 1567.0), xs, xs])
    be, bn = proj.forward(*ref.forward(by, bx))
    slack = ((be.min() - f.e_left) / f.res, f.width - (be.max() - f.e_left) / f.res, (f.n_top - bn.max()) / f.res, f.height - (f.n_top - bn.min()) / f.res)
    print(f"pixels between the border's box and the frame: left {slack[0]:.3f}, right {slack[1]:.3f}, top {slack[2]:.3f}, bottom {slack[3]:.3f}")
    assert all(s >= -1e-6 for s in slack) and slack[0] <= 1 and slack[1] <= 1 + 3 and slack[2] <= 1 and slack[3] <= 1
    # the line times are the map layer's
    want = MP.fit_time(p.place, p.sinfo)
    r = g.passes[0]
    assert (r.row_period, r.s0, r.rows_fit, r.lines, r.date) == (want.row_period, want.s0, PU_.POLAR_ROWS, lines, 19822)
    wld = [float(v) for v in f.world_file().split()]
    assert wld == [f.res, 0, 0, -f.res, f.e_left + f.res / 2, f.n_top - f.res / 2]
    prj = f.prj()
    print(prj.strip())
    assert prj.startswith('PROJCS[') and 'PROJECTION["Polar_Stereographic"]' in prj and 'PARAMETER["latitude_of_origin",70]' in prj
    assert f'PARAMETER["central_meridian",{f.lon0_deg:g}]' in prj and 'PARAMETER["false_easting",0]' in prj and 'PARAMETER["false_northing",0]' in prj and 'UNIT["metre",1]' in prj


def test_pole_and_meridian_choice():
    from meteor_demod_amd import polar as P
    south, ref = PU_.polar_pass(PU_.SOUTH_U)
    lat_c, lon_c = ref.forward((8 * PU_.POLAR_ROWS - 1) / 2, 783.5)
    f = P.grid([south], metres_per_pixel=2000).frame
    print(f"the pass from {PU_.SOUTH_U} degrees: centre pixel at {lat_c:.3f}, {lon_c:.3f}: pole {f.pole}, lat_ts {f.lat_ts_deg}, lon0 {f.lon0_deg}")
    assert lat_c < 0 and f.pole == -1 and f.lat_ts_deg == -70.0 and f.lon0_deg == np.floor(lon_c + 0.5)
    assert 'PARAMETER["latitude_of_origin",-70]' in f.prj()
    short = PU_.polar_pass(PU_.SHORT_U, PU_.SHORT_ROWS)[0]
    for opts, want in ((dict(lon0_deg=-33.25), -33.25), (dict(lon0_deg=270.0), -90.0), (dict(lon0_deg="auto", pole=1, lat_ts_deg=90), None)):
        g = P.grid([short], metres_per_pixel=4000, **opts).frame
        assert g.pole == 1 and (want is None or g.lon0_deg == want) and g.lat_ts_deg == opts.get("lat_ts_deg", 70)


def test_refusals():
    from meteor_demod_amd import _capi, polar as P
    top, short, south = PU_.polar_pass()[0], PU_.polar_pass(PU_.SHORT_U, PU_.SHORT_ROWS)[0], PU_.polar_pass(PU_.SOUTH_U)[0]
    equator = PU_.plain_pass(120, MU.mid_latitude_s0(-5.0))
    for word, fn in (("no pass", lambda: P.grid([])), ("1 .. 8", lambda: P.grid([short] * 9)), ("100 .. 100000", lambda: P.grid([short], metres_per_pixel=99)),
                     ("100 .. 100000", lambda: P.grid([short], metres_per_pixel=100001)), ("pole is 2", lambda: P.grid([short], pole=2)),
                     ("standard parallel", lambda: P.grid([short], lat_ts_deg=0)), ("standard parallel", lambda: P.grid([short], lat_ts_deg=91)),
                     ("central meridian", lambda: P.grid([short], lon0_deg=361)), ("nodes_on_host", lambda: P.grid([short], nodes_on_host=2)),
                     ("projection 1", lambda: P.grid([short], projection=1)), ("latitude / longitude grid", lambda: P.grid([short], pole=-1)),
                     ("latitude / longitude grid", lambda: P.grid([equator], pole=1)), ("latitude / longitude grid", lambda: P.grid([short, south], metres_per_pixel=4000)),
                     ("does not see the Earth", lambda: P.grid([short], scan_deg=130)), ("fits", lambda: P.grid([top], metres_per_pixel=300)),
                     ("scan side", lambda: P.grid([short], side=0)), ("stretch", lambda: P.grid([short], stretch=3)), ("blend", lambda: P.grid([short], blend=2)),
                     ("piece_lines", lambda: P.grid([short], piece_lines=24)), ("no element set", lambda: P.grid([PU_.plain_pass(5, MU.mid_latitude_s0(88.0), "hello\n")])),
                     ("no placed packet", lambda: P.grid([type(short)(short.tle_text, short.images, short.filled, short.place[:0], short.sinfo[:0])]))):
        with pytest.raises(_capi.MdemodError) as e:
            fn()
        print(f"{word}: '{e.value.detail}'")
        assert e.value.code == _capi.MDEMOD_ERR_PARAM and word in e.value.detail
    with pytest.raises(_capi.MdemodError) as e:
        P.grid([top], metres_per_pixel=300)
    fit = int(re.search(r"resolution of (\d+) fits", e.value.detail).group(1))
    ok = P.grid([top], metres_per_pixel=fit).frame
    print(f"at 300 m refused, the resolution named is {fit} m: {ok.width} x {ok.height}")
    assert ok.width <= 8192 and ok.height <= 16384 and 300 < fit < 1000 and max(ok.width / 8192, ok.height / 16384) > 0.9


# ----------------------------------------------------------------------------------------------------------------- nodes
def _against_numpy(nodes, frame, ref, lines, pick=None):
    e, n = PU_.node_centres(frame)
    got = nodes.reshape(-1, 2)
    e, n = e.reshape(-1), n.reshape(-1)
    if pick is not None:
        e, n, got = e[pick], n[pick], got[pick]
    y, x = PR.inverse_pass(ref, PU_.proj_of(frame), e, n, lines)
    none = PU_.missing(got)
    both = ~none & np.isfinite(y)
    ex, ey = np.abs(got[both, 0] - 256 * x[both]), np.abs(got[both, 1] - 256 * y[both])
    lat, _ = PU_.proj_of(frame).inverse(e, n)
    return none, np.isnan(y), ex.max(), ey.max(), (90.0 - np.abs(lat))


def test_host_nodes_against_the_numpy_inverse():
    """The 600-row pass at 1000 m (3000 nodes drawn from its 116 592) and the 40 lines from 88 degrees at 4000 m (all 495 nodes,
    the pole inside the swath): 1 unit of 1/256 pixel, and the same nodes missing."""
    g, ref = polar_grid(), PU_.polar_pass()[1]
    pick = np.random.default_rng(9).choice(g.nodes[0].size // 2, 3000, replace=False)
    none, ref_none, ex, ey, _ = _against_numpy(g.nodes[0], g.frame, ref, 8 * PU_.POLAR_ROWS, pick)
    print(f"600 rows at 1000 m: {int(none.sum())} of {none.size} nodes missing ({int(ref_none.sum())} in numpy); worst difference {ex:.3f} in X, {ey:.3f} in Y")
    assert np.array_equal(none, ref_none) and 0 < none.sum() < none.size and ex <= 1.0 and ey <= 1.0
    g, ref = polar_grid(PU_.SHORT_U, PU_.SHORT_ROWS, 4000.0), PU_.polar_pass(PU_.SHORT_U, PU_.SHORT_ROWS)[1]
    none, ref_none, ex, ey, off = _against_numpy(g.nodes[0], g.frame, ref, 8 * PU_.SHORT_ROWS)
    print(f"40 lines at 4000 m: {g.nodes.shape[1]} x {g.nodes.shape[2]} nodes, {int(none.sum())} missing ({int(ref_none.sum())} in numpy); worst difference {ex:.3f} in X, "
          f"{ey:.3f} in Y; the nearest node stands {off.min():.3f} degrees from the pole")
    assert np.array_equal(none, ref_none) and ex <= 1.0 and ey <= 1.0 and g.nodes.shape[1:] == (45, 11, 2)


def test_host_nodes_at_the_pole():
    """A frame laid so that node (1, 2) is the pole itself and its neighbours stand 16 pixels of 100 m from it (0.014 degrees), through
    model_nodes."""
    from meteor_demod_amd import polar as P
    p, ref = PU_.polar_pass(PU_.SHORT_U, PU_.SHORT_ROWS)
    res = 100.0
    frame = P.Frame(64, 48, res, -32.5 * res, 16.5 * res, 1, 70.0, 47.0)
    g = P.model_nodes([p], frame, metres_per_pixel=res)
    assert g.frame == frame
    none, ref_none, ex, ey, off = _against_numpy(g.nodes[0], frame, ref, 8 * PU_.SHORT_ROWS)
    print(f"{none.size} nodes, {int(none.sum())} missing; {int((off < 0.05).sum())} closer than 0.05 degrees to the pole, the nearest at {off.min():.2e}; worst difference "
          f"{ex:.3f} in X, {ey:.3f} in Y; the pole is seen from pixel {(g.nodes[0][1, 2] / 256).tolist()}")
    assert off.reshape(g.nodes.shape[1:3])[1, 2] == 0.0 and (off < 0.05).sum() >= 9 and not none.any() and not ref_none.any() and ex <= 1.0 and ey <= 1.0
    # the frame of `grid` gives the same nodes through either entry
    own = polar_grid(PU_.SHORT_U, PU_.SHORT_ROWS, 4000.0)
    again = P.model_nodes([p], own.frame, metres_per_pixel=4000)
    assert np.array_equal(again.nodes, own.nodes)


# Worst difference between the interpolated and the exact source coordinates, in source pixels, over the pixels of 320 cells of the
# 600-row polar pass at 1000 m that fall inside the picture (profiles/polar.md): measured 0.0317, in X.  The bar is 1.5 times that,
# as the map layer's: it covers other orbits of the same family.
GRID_COST_BAR = 1.5 * 0.0317


def test_what_the_16_pixel_grid_costs():
    g, ref = polar_grid(), PU_.polar_pass()[1]
    lines = 8 * PU_.POLAR_ROWS
    rng = np.random.default_rng(16)
    n = g.nodes[0].astype(np.int64)
    whole = ~PU_.missing(n)
    cells = np.argwhere(whole[:-1, :-1] & whole[1:, :-1] & whole[:-1, 1:] & whole[1:, 1:])
    cells = cells[rng.choice(len(cells), 320, replace=False)]
    p, q = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    a, b = cells[:, 0][:, None, None], cells[:, 1][:, None, None]
    w = [(16 - p) * (16 - q), p * (16 - q), (16 - p) * q, p * q]
    corner = [n[a, b], n[a + 1, b], n[a, b + 1], n[a + 1, b + 1]]
    X = (sum(w[k] * corner[k][..., 0] for k in range(4)) + 128) >> 8
    Y = (sum(w[k] * corner[k][..., 1] for k in range(4)) + 128) >> 8
    e, nn = g.frame.centres(16 * a + p, 16 * b + q)
    y, x = PR.inverse_pass(ref, PU_.proj_of(g.frame), e, nn, lines, steps=8, seed=(Y / 256.0, X / 256.0))
    inside = (X >= 0) & (X <= 1567 * 256) & (Y >= 0) & (Y <= (lines - 1) * 256) & np.isfinite(y)
    worst_x, worst_y = np.abs(X / 256 - x)[inside].max(), np.abs(Y / 256 - y)[inside].max()
    print(f"1000 m: {int(inside.sum())} pixels of 320 cells inside the picture, worst difference {max(worst_x, worst_y):.4f} source pixel (X {worst_x:.4f}, Y {worst_y:.4f}), "
          f"bar {GRID_COST_BAR:.4f}")
    assert inside.sum() > 20000 and np.isfinite(y).sum() == y.size and max(worst_x, worst_y) <= GRID_COST_BAR


# ----------------------------------------------------------------------------------------------------------------- scene
SQUARE, SCENE_ROWS, SCENE_U, SCENE_RES = 2.0, 160, 68.0, 2000.0
B_RAAN, B_LATER = 170.0, 12


@functools.lru_cache(maxsize=None)
def scene_passes():
    """Pass A: 160 strip rows that run over the top of the orbit, painted from squares of 2 degrees, 10 % of its strips lost.
    Pass B: the same orbit with its node 20 degrees further east, 12 row periods later, with its own losses.  (passes, marked)."""
    from meteor_demod_amd import mosaic as M
    rng = np.random.default_rng(41)
    out, marked = [], None
    for text, later in ((MU.tle_text(), 0), (MU.with_raan(B_RAAN), B_LATER)):
        s0 = MU.mid_latitude_s0(SCENE_U) + later * MU.ROW_PERIOD
        ref = MU.ref_pass(SCENE_ROWS, s0=s0, text=text)
        if marked is None:
            lat, lon = ref.forward(4 * SCENE_ROWS, 600.0)
            marked = (float(SQUARE * np.floor(lat / SQUARE)), float(SQUARE * np.floor(lon / SQUARE)))
        place, info = MU.packets(SCENE_ROWS, s0, keep=rng.random((SCENE_ROWS, 3, 14)) >= 0.1)
        out.append(M.Pass(text, MU.paint(ref, SCENE_ROWS, SQUARE, marked), MU.filled_of(place, SCENE_ROWS), place, info))
    return out, marked


def check_scene(m, marked, label):
    """Every valid byte at least 3 output pixels from a square's edge is the scene's level at the pixel centre's (lat, lon).  A
    square of 2 degrees is 222 km high and 222 km cos(lat) wide, 111 by 111 cos(lat) pixels of 2000 m: at 85 degrees 111 x 9.7, of
    which (1 - 6 / 111) (1 - 6 / 9.7) = 0.36 is kept, at 80 degrees 0.65, at 70 degrees 0.80; the swaths reach the pole but most of
    their area lies below 80 degrees: at least 40 % are kept."""
    f = m.frame
    i, j = np.meshgrid(np.arange(m.height), np.arange(m.width), indexing="ij")
    lat, lon = PU_.proj_of(f).inverse(*f.centres(i, j))
    d_lat, d_lon = MU.edge_distance(lat, lon, SQUARE)
    per_deg = 111.0e3 / f.res
    far = (d_lat * per_deg >= 3.0) & (d_lon * per_deg * np.cos(np.radians(lat)) >= 3.0)
    seen = 0
    for pl, ch in enumerate(m.select):
        ok = ((m.valid >> pl) & 1).astype(bool)
        want = MU.scene(lat, lon, ch, SQUARE, marked)
        wrong = ok & far & (m.pixels[..., pl] != want)
        share = (ok & far).sum() / max(ok.sum(), 1)
        print(f"{label}, plane {pl}: {int(ok.sum())} valid pixels, {100 * share:.1f} % kept, {int(wrong.sum())} wrong")
        assert not wrong.any() and share >= 0.4 and ok.sum() > 0.1 * ok.size
        seen += int((ok & far & (want == MU.MARKED_LEVEL)).sum())
    print(f"{label}: {seen} bytes of the marked square")
    assert seen > 100


@functools.lru_cache(maxsize=None)
def scene_model(n_passes, blend="feather", piece_lines=64, select=(2, 1, 0)):
    from meteor_demod_amd import polar as P
    passes, _ = scene_passes()
    return P.model_host(list(passes[:n_passes]), select, stretch=0, metres_per_pixel=SCENE_RES, blend=blend, piece_lines=piece_lines)


def test_scene_through_the_cpu_path():
    from meteor_demod_amd import mosaic as M, polar as P
    passes, marked = scene_passes()
    m = scene_model(1)
    print(f"{m.width} x {m.height}, {100 * m.valid_share:.1f} % valid, marked square at {marked}")
    check_scene(m, marked, "one pass")
    assert m.nodes_on_host and m.blend == 0 and m.passes[0].limits == [(0, 255)] * 3 and m.passes[0].date == 19822 and m.passes[0].rows_fit == SCENE_ROWS
    g = P.grid(passes[:1], metres_per_pixel=SCENE_RES)
    assert g.frame == m.frame and np.array_equal(g.nodes, m.nodes)
    # the picture is the mosaic layer's model blend through these nodes
    ident = np.arange(256, dtype=np.uint8)[None].repeat(3, 0)
    out, val, cov = M.model_blend([(passes[0].images, passes[0].filled, ident, m.nodes[0])], (2, 1, 0), m.width, m.height, "feather", valid=True, cover=True)
    assert np.array_equal(out, m.pixels) and np.array_equal(val, m.valid) and np.array_equal(cov, m.cover)
    whole = scene_model(1, piece_lines=16384)
    assert np.array_equal(whole.pixels, m.pixels) and np.array_equal(whole.valid, m.valid) and np.array_equal(whole.cover, m.cover)


@pytest.mark.parametrize("blend", ["feather", "best"])
def test_two_passes_overlap(blend):
    passes, marked = scene_passes()
    m = scene_model(2, blend)
    print(f"{m.width} x {m.height}, {100 * m.valid_share:.1f} % valid, {100 * m.overlap_share:.1f} % seen by both; covered {[r.covered for r in m.passes]}")
    check_scene(m, marked, f"two passes, {blend}")
    assert m.nodes.shape[0] == 2 and m.overlap_pixels == (m.cover == 3).sum() and set(np.unique(m.cover)) == {0, 1, 2, 3}
    assert blend == "best" or m.overlap_share > 0.1
    assert all(r.covered == np.count_nonzero(m.cover & (1 << k)) and r.covered > 0.1 * m.cover.size for k, r in enumerate(m.passes))
    assert abs(m.passes[1].utc0 - m.passes[0].utc0 - B_LATER * MU.ROW_PERIOD) < 1e-6


# -------------------------------------------------------------------------------------------------- vertices and graticule
def test_vertices_against_the_python_bisection():
    from meteor_demod_amd import polar as P
    f = polar_grid().frame
    proj = PU_.proj_of(f)
    rng = np.random.default_rng(12)
    lon, lat, first = [], [], [0]
    for _ in range(40):                                                            # random walks in the northern hemisphere, across +-180
        k = int(rng.integers(2, 9))
        lo, la = rng.uniform(-180, 180), rng.uniform(50, 89)
        for _ in range(k):
            lon.append((lo + 180.0) % 360.0 - 180.0); lat.append(float(np.clip(la, 30.0, 90.0)))
            lo, la = lo + rng.uniform(-40, 40), la + rng.uniform(-8, 8)
        first.append(len(lon))
    # a parallel in one segment of 170 degrees, a meridian through the pole, a line that dips into the other hemisphere and comes back
    lon += [f.lon0_deg - 85.0, f.lon0_deg + 85.0]; lat += [80.0, 80.0]; first.append(len(lon))
    lon += [10.0, 10.0, -170.0]; lat += [70.0, 90.0, 70.0]; first.append(len(lon))
    lon += [0.0, 5.0, 10.0, 15.0, 20.0, 25.0, 30.0]; lat += [10.0, 5.0, -1.0, 4.0, 8.0, 0.0, 3.0]; first.append(len(lon))
    x, y, fi = P.vertices(f, lon, lat, first)
    rx, ry, rf = PR.vertices(proj, f, lon, lat, first)
    print(f"{len(first) - 1} polylines of {len(lon)} vertices become {len(fi) - 1} of {len(x)} (python: {len(rf) - 1} of {len(rx)})")
    assert fi.tolist() == rf and len(x) == len(rx)
    d = max(np.abs(x - np.array(rx)).max(), np.abs(y - np.array(ry)).max())
    print(f"worst difference {d} units")
    assert d <= 1 and len(fi) - 1 == len(first) - 1 + 1                            # the dipping line comes out as two: 0 .. 5 and 15 .. 20; 30 alone is dropped
    ends = [PR.fixed(proj, f, lo, la) for lo, la in ((0.0, 10.0), (5.0, 5.0), (15.0, 4.0), (20.0, 8.0))]
    for (ex, ey), at in zip(ends, (fi[-3], fi[-2] - 1, fi[-2], fi[-1] - 1)):
        assert abs(x[at] - ex) <= 1 and abs(y[at] - ey) <= 1
    with pytest.raises(Exception):
        P.vertices(f, [0.0, 1.0], [91.0, 50.0], [0, 2])


def test_graticule_parallel_is_an_arc():
    """Every vertex of the 80 degree parallel of a 5 degree graticule stands on its circle, and so does every chord's midpoint, to the
    64 units the bisection allows plus 2 of rounding."""
    from meteor_demod_amd import polar as P
    f = polar_grid().frame
    lon, lat, first, step = P.graticule(f, 5.0)
    assert step == 5.0
    proj = PU_.proj_of(f)
    inside_pole = f.e_left <= 0 <= f.e_left + f.width * f.res and f.n_top - f.height * f.res <= 0 <= f.n_top
    par = [l for l in range(len(first) - 1) if lat[first[l]] == lat[first[l + 1] - 1]]
    mer = [l for l in range(len(first) - 1) if l not in par]
    print(f"{len(par)} parallels at {sorted({float(lat[first[l]]) for l in par})}, {len(mer)} meridians; the pole lies inside: {inside_pole}")
    assert inside_pole and len(mer) == 72 and max(lat[first[l + 1] - 1] for l in mer) == 90.0
    l80 = next(l for l in par if lat[first[l]] == 80.0)
    sl = slice(int(first[l80]), int(first[l80 + 1]))
    assert abs((lon[sl][-1] - lon[sl][0]) - 360.0) < 1e-9                          # the full circle
    x, y, fi = P.vertices(f, lon[sl], lat[sl], [0, sl.stop - sl.start])
    cx, cy = PR.fixed(proj, f, 0.0, 90.0)
    radius = 256.0 * proj.scale * float(PR.t_of(np.radians(80.0))) / f.res
    r_vertex = np.hypot(x - cx, y - cy)
    r_mid = np.hypot((x[1:] + x[:-1]) / 2 - cx, (y[1:] + y[:-1]) / 2 - cy)
    print(f"{sl.stop - sl.start} vertices become {len(x)}; radius {radius:.1f} units; vertices off by at most {np.abs(r_vertex - radius).max():.2f}, chord midpoints by "
          f"{np.abs(r_mid - radius).max():.2f}")
    assert len(fi) == 2 and np.abs(r_vertex - radius).max() <= 2 and np.abs(r_mid - radius).max() <= 64 + 2
    # automatic: the smallest step whose parallels stand 128 pixels apart at the middle of the extent (the pole to the farthest edge pixel)
    _, _, _, auto = P.graticule(f, 0.0)
    i, j = np.meshgrid([0, f.height - 1], [0, f.width - 1], indexing="ij")
    mid = 0.5 * (90.0 + np.abs(proj.inverse(*f.centres(i, j))[0]).min())
    apart = {s: proj.scale * float(PR.t_of(np.radians(min(90.0, mid + s / 2) - s)) - PR.t_of(np.radians(min(90.0, mid + s / 2)))) / f.res for s in (1, 2, 5, 10, 15, 30)}
    print(f"automatic step {auto:g}; at {mid:.2f} degrees parallels stand { {s: round(v, 1) for s, v in apart.items()} } pixels apart")
    assert auto == min(s for s in apart if apart[s] >= 128)


# --------------------------------------------------------------------------------------------------------------- binding
HEADER = ROOT / "include" / "meteor_demod_amd_polar.h"
ENTRIES = ["mdemod_polar_default_opts", "mdemod_polar_forward", "mdemod_polar_inverse", "mdemod_polar_grid", "mdemod_polar_grid_free", "mdemod_polar_nodes_work_bytes",
           "mdemod_polar_nodes_device", "mdemod_polar_compose_host", "mdemod_polar_free", "mdemod_polar_graticule", "mdemod_polar_lines_free", "mdemod_polar_vertices",
           "mdemod_polar_points_free", "mdemod_polar_draw_host", "mdemod_polar_world_file", "mdemod_polar_prj"]


def _header_entries():
    return re.findall(r"^\s*(?:int|void|uint64_t)\s+(mdemod_\w+)\s*\(", HEADER.read_text(), re.M)


def test_polar_entries_exported_and_bound():
    from meteor_demod_amd import _capi, map as MP, mosaic as M, overlay, picture, polar as P
    names = _header_entries()
    assert sorted(names) == sorted(ENTRIES)
    lib = P.lib()
    for n in names + list(P.MODEL_SIGNATURES):
        assert hasattr(lib, n), n
    assert sorted(P.SIGNATURES) == sorted(names) and sorted(P.MODEL_SIGNATURES) == ["mdemod_polar_model_host", "mdemod_polar_model_nodes"]
    others = list(_capi.SIGNATURES) + list(picture.SIGNATURES) + list(MP.SIGNATURES) + list(MP.MODEL_SIGNATURES) + list(M.SIGNATURES) + list(M.MODEL_SIGNATURES) + list(overlay.SIGNATURES)
    assert not any("polar" in n for n in others)
    text = HEADER.read_text()
    assert not any(w in text for w in ("mdemod_map_", "mdemod_mosaic_", "mdemod_overlay_")) and '#include "meteor_demod_amd_picture.h"' in text
    for h in (ROOT / "include").glob("*.h"):
        if h.name != HEADER.name:
            assert "mdemod_polar_" not in h.read_text(), h.name
    assert _capi.lib().mdemod_abi_version() == 5
    for fn in ("compose", "images_to_polar", "grid", "nodes_device", "graticule", "vertices", "world_file", "prj", "model_host", "model_nodes", "forward", "inverse"):
        assert callable(getattr(P, fn))
    o = P.make_opts()
    assert (o.scan_deg, o.time_offset, o.row_period, o.metres_per_pixel, o.lat_ts_deg, o.side, o.pole, o.stretch, o.clip_low, o.clip_high, o.piece_lines, o.blend,
            o.nodes_on_host, o.projection) == (110.0, 10800.0, 8 / 6.5, 1000.0, 70.0, 1, 0, 1, 5, 5, 0, 0, 0, 0) and np.isnan(o.lon0_deg)
    assert P.make_opts(blend="best").blend == 1
    with pytest.raises(TypeError):
        P.make_opts(px_per_deg=3)


def test_polar_int_entries_are_function_try_blocks():
    from meteor_demod_amd import polar as P
    found = 0
    entries = set(_header_entries()) | set(P.MODEL_SIGNATURES)
    for src in (ROOT / "meteor_demod_amd" / "csrc" / "polar.hip", ROOT / "meteor_demod_amd" / "csrc" / "polar_host.cpp"):
        text = src.read_text()
        for m in re.finditer(r"^int\n(mdemod_\w+)\(", text, re.M):
            assert m.group(1) in entries, m.group(1)
            found += 1
            body = text[m.end():]
            assert body[: body.index("{")].rstrip().endswith("try"), f"{src.name}: {m.group(1)} is not a function-try-block"
            assert body[body.index("{"):].lstrip("{ ").startswith("MDEMOD_API_ENTER"), m.group(1)
            assert body[body.index("\n}"):].startswith("\n} MDEMOD_API_CATCH"), f"{src.name}: {m.group(1)} does not end in MDEMOD_API_CATCH"
    assert found == 3 + 9, found
    listed = (ROOT / "meteor_demod_amd" / "csrc" / "polar_host.h").read_text()
    assert all(n in listed for n in P.MODEL_SIGNATURES)
    # the host side stays free of the GPU runtime, and the solver and the blend exist once
    host = (ROOT / "meteor_demod_amd" / "csrc" / "polar_host.cpp").read_text() + listed + (ROOT / "meteor_demod_amd" / "csrc" / "polar_proj.h").read_text()
    assert "hip_runtime" not in host and "hip_host.h" not in host and "map_nodes_at" in host
    device = (ROOT / "meteor_demod_amd" / "csrc" / "polar.hip").read_text()
    # the picture goes through the mosaic layer's own back ends: one kernel here, no band, table or histogram step of its own
    assert '#include "mosaic_device.h"' in device and device.count("__global__") == 1
    assert not re.search(r"\b(histogram|tables|band)\(", device)
    assert not re.search(r":\s*(public\s+)?MosaicBackend\b", (ROOT / "meteor_demod_amd" / "csrc" / "polar_host.cpp").read_text())


def test_cli_without_polar_layer_links_and_refuses(tmp_path):
    """The C host against tests/sanitize/stub_backend.c (which has no polar layer): it links, --help lists the four options, and
    --map-proj stereo exits with status 1 saying which layer the library lacks, and writes nothing.  Against the real library the
    options are refused before anything is demodulated where they make no sense."""
    import frames_util as U
    exe = tmp_path / "cli_stub"
    r = subprocess.run(["gcc", "-std=gnu11", "-O1", "-Wall", "-I", str(ROOT / "include"), str(ROOT / "host" / "meteor_demod_amd.c"),
                        str(ROOT / "tests" / "sanitize" / "stub_backend.c"), "-pthread", "-lm", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    h = subprocess.run([str(exe), "--help"], capture_output=True, text=True)
    assert h.returncode == 0 and all(w in h.stderr for w in ("--map-proj <p>", "--map-res <metres>", "--map-lon0 <deg|auto>", "--map-lat-ts <deg>"))
    wav = tmp_path / "in.wav"
    wav.write_bytes(U.wav_bytes(288000, np.zeros((16384, 2), dtype=np.int16)))
    tle = MU.GOLDEN / "map_tle.txt"
    r = subprocess.run([str(exe), "-q", "-o", str(tmp_path / "out.s"), "--image", "--map", str(tle), "--map-proj", "stereo", str(wav)], capture_output=True, text=True, cwd=tmp_path)
    print(r.stderr.strip())
    assert r.returncode == 1 and "no polar layer" in r.stderr and "unrecognized" not in r.stderr, r.stderr
    assert r.stdout == "" and sorted(p.name for p in tmp_path.iterdir()) == ["cli_stub", "in.wav"]
    cli_exe = ROOT / "meteor_demod_amd" / "lib" / "meteor_demod_amd"
    for flags, word in ((("--image", "--map-proj", "stereo"), "only with --map"), (("--image", "--map", str(tle), "--map-res", "2000"), "only with --map-proj stereo"),
                        (("--image", "--map", str(tle), "--map-proj", "stereo", "--map-scale", "50"), "not with --map-proj stereo"),
                        (("--image", "--map", str(tle), "--map-proj", "mercator"), "latlon or stereo"),
                        (("--image", "--map", str(tle), "--map-proj", "stereo", "--map-res", "50"), "100 .. 100000"),
                        (("--image", "--map", str(tle), "--map-proj", "stereo", "--map-lon0", "400"), "-360 .. 360"),
                        (("--image", "--map", str(tle), "--map-proj", "stereo", "--map-lat-ts", "0"), "0 < .. <= 90")):
        r = subprocess.run([str(cli_exe), "-q", "-B", *flags, str(wav)], capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == 1 and word in r.stderr and r.stdout == "", (flags, r.stderr)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["cli_stub", "in.wav"]


def test_polar_struct_layouts(tmp_path):
    import ctypes as C
    from meteor_demod_amd import polar as P
    names = ["opts", "pass", "timing", "frame", "solver", "nodes", "result", "lines", "points", "style", "drawn"]
    offs = [("style", "inside_only"), ("drawn", "items"),("opts", "reserved"), ("pass", "n_desc"), ("timing", "lines"), ("frame", "lon0_deg"), ("solver", "table"), ("nodes", "nodes"), ("nodes", "solver"),
            ("result", "utc0"), ("result", "nodes"), ("lines", "step_deg"), ("points", "n_points")]
    args = ", ".join([f"sizeof(mdemod_polar_{n})" for n in names] + [f"offsetof(mdemod_polar_{s}, {f})" for s, f in offs])
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "meteor_demod_amd_polar.h"\nint main(void){printf("' + "%zu " * (len(names) + len(offs)) + '\\n", ' + args +
           "); return 0;}")
    (tmp_path / "s.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")], check=True)
    out = [int(x) for x in subprocess.run([str(tmp_path / "s")], capture_output=True, text=True, check=True).stdout.split()]
    types = dict(opts=P.MdemodPolarOpts, timing=P.MdemodPolarTiming, frame=P.MdemodPolarFrame, solver=P.MdemodPolarSolver, nodes=P.MdemodPolarNodes,
                 result=P.MdemodPolarResult, lines=P.MdemodPolarLines, points=P.MdemodPolarPoints, style=P.MdemodPolarStyle, drawn=P.MdemodPolarDrawn)
    types["pass"] = P.MdemodPolarPass
    print(out)
    assert out == [C.sizeof(types[n]) for n in names] + [getattr(types[s], f).offset for s, f in offs]
