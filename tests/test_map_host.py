"""CPU tests of the map layer (include/meteor_demod_amd_map.h): the TLE parser, the forward function against the numpy model of
map_ref.py and against physics that does not come from its formulas, the time fit, the nodes against the numpy model's own inverse,
what the 16-pixel grid costs, the host model of the warp on hand-made node grids, and a scene of latitude / longitude squares
through the whole CPU path.  Every test prints the figures it asserts on."""
from __future__ import annotations

import functools
import re

import numpy as np
import pytest

import map_ref as R
from conftest import ROOT
import map_util as MU
import picture_util as PU

ROWS = 600


@functools.lru_cache(maxsize=None)
def _pass(rows=ROWS):
    """(tle, timing, numpy pass) of the clean mid-latitude pass."""
    from meteor_demod_amd import map as M
    place, info = MU.packets(rows, MU.mid_latitude_s0())
    tle = M.parse_tle(MU.tle_text())
    return tle, M.fit_time(place, info), MU.ref_pass(rows)


@functools.lru_cache(maxsize=None)
def _grid(scale=100):
    from meteor_demod_amd import map as M
    tle, timing, ref = _pass()
    return M.grid(tle, timing, 8 * ROWS, px_per_deg=scale)


def _centres(g, i, j):
    return g.lat_top - (np.asarray(i) + 0.5) / g.sy, g.lon_left + (np.asarray(j) + 0.5) / g.sx


# ------------------------------------------------------------------------------------------------------------------- TLE
def test_tle_fields_and_refusals():
    from meteor_demod_amd import _capi, map as M
    text = MU.tle_text()
    t, o = M.parse_tle(text), MU.orbit()
    print(t.norad, t.epoch_day, t.epoch_sec, t.inclination_deg, t.raan_deg, t.eccentricity, t.argp_deg, t.mean_anomaly_deg, t.mean_motion)
    assert (t.norad, t.epoch_day, t.epoch_sec) == (99001, o.epoch_day, 43200.0) and t.epoch_day == 19822                # 2024-04-09
    assert (t.inclination_deg, t.raan_deg, t.eccentricity, t.argp_deg, t.mean_anomaly_deg, t.mean_motion) == (98.77, 150.0, 0.0005, 90.0, 270.0, 14.23)
    name, l1, l2 = text.splitlines()
    assert M.parse_tle(l1 + "\r\n" + l2).norad == 99001                                # no name line, CR LF
    both = text + MU.second_set()
    assert M.parse_tle(both).raan_deg == 150.0 and M.parse_tle(both, 99002).raan_deg == 200.0 and M.parse_tle(both, 99002).norad == 99002
    flip = lambda line, at: line[:at] + str((int(line[at]) + 1) % 10) + line[at + 1:]
    for word, bad in (("checksum of line 1", "\n".join([flip(l1, 68), l2])), ("checksum of line 2", "\n".join([l1, flip(l2, 68)])),
                      ("checksum of line 2", "\n".join([l1, flip(l2, 12)])), ("short", "\n".join([l1[:60], l2])), ("short", "\n".join([l1, l2[:68]])),
                      ("catalogue number", "\n".join([R.edit(l1, 3, "     "), l2])), ("catalogue numbers", "\n".join([l1, R.edit(l2, 3, "99003")])),
                      ("no line 2", "\n".join([l1, "3" + l2[1:]])), ("without its line 1", "\n".join(["3" + l1[1:], l2])), ("no element set", "hello\n"),
                      ("no element set", ""), ("not a number", "\n".join([l1, R.edit(l2, 9, "  98.7x ")]))):
        with pytest.raises(_capi.MdemodError) as e:
            M.parse_tle(bad)
        print(f"{word}: '{e.value.detail}'")
        assert e.value.code == _capi.MDEMOD_ERR_PARAM and word in e.value.detail
    with pytest.raises(_capi.MdemodError) as e:
        M.parse_tle(both, 12345)
    assert "12345" in e.value.detail


# ------------------------------------------------------------------------------------------------------- forward function
def test_forward_equals_the_numpy_model():
    """2000 random pixels inside and around a pass of 600 strip rows, some beyond the horizon.  1e-6 degree is 0.1 m: rounding in
    this chain is about 1e-8 degree (the GMST product is near 3e6 degrees, the arguments of the sines near 1e3 radians), a pixel is 1e-2 degree."""
    from meteor_demod_amd import map as M
    tle, timing, ref = _pass()
    rng = np.random.default_rng(5)
    y, x = rng.uniform(-300, 8 * ROWS + 300, 2000), rng.uniform(-160, 1727, 2000)
    for side in (1, -1):
        lat, lon = M.geolocate(tle, timing, y, x, side=side)
        ref.side = side
        want_lat, want_lon = ref.forward(y, x)
        ref.side = 1
        hidden = np.isnan(lat)
        err = max(np.nanmax(np.abs(lat - want_lat)), np.nanmax(np.abs((lon - want_lon + 180) % 360 - 180)))
        print(f"side {side}: {int(hidden.sum())} of 2000 not visible, worst difference {err:.3e} degree")
        assert np.array_equal(hidden, np.isnan(want_lat)) and np.array_equal(hidden, np.isnan(lon)) and 0 < hidden.sum() < 400
        assert err < 1e-6


def _ecef(lat, lon):
    la, lo = np.radians(lat), np.radians(lon)
    n = R.RE / np.sqrt(1 - R.E2 * np.sin(la) ** 2)
    return np.stack([n * np.cos(la) * np.cos(lo), n * np.cos(la) * np.sin(lo), n * (1 - R.E2) * np.sin(la)], -1)


def test_forward_physics():
    from meteor_demod_amd import map as M
    tle, timing, ref = _pass()
    y = np.linspace(0, 8 * ROWS - 1, 50)
    # the nadir column looks along -r: its footprint has r's longitude, and its geocentric direction is r
    lat, lon = M.geolocate(tle, timing, y, np.full(50, 783.5))
    r, _, _ = ref.orbit.frame(ref.date, ref.sec(y))
    p = _ecef(lat, lon)
    off = np.abs((lon - np.degrees(np.arctan2(r[:, 1], r[:, 0])) + 180) % 360 - 180).max()
    turn = np.abs(p / np.linalg.norm(p, axis=1)[:, None] - r).max()
    print(f"nadir: longitude off r by {off:.2e} degree, direction off r by {turn:.2e}")
    assert off < 1e-6 and turn < np.radians(1e-6)                                  # the bar of the comparison above, as an angle
    # the README's swath: about 2800 km between the footprints of columns 0 and 1567
    a, b = _ecef(*M.geolocate(tle, timing, y, np.zeros(50))), _ecef(*M.geolocate(tle, timing, y, np.full(50, 1567.0)))
    rad = 0.5 * (np.linalg.norm(a, axis=1) + np.linalg.norm(b, axis=1))
    swath = rad * np.arccos(np.clip((a * b).sum(1) / np.linalg.norm(a, axis=1) / np.linalg.norm(b, axis=1), -1, 1))
    print(f"swath {swath.min():.0f} .. {swath.max():.0f} km")
    assert (np.abs(swath - 2800.0) < 0.05 * 2800.0).all()
    # side = -1 mirrors the swath about the track
    x = np.linspace(0, 1567, 50)
    one, two = M.geolocate(tle, timing, y, x, side=-1), M.geolocate(tle, timing, y, 1567.0 - x)
    assert np.abs(one[0] - two[0]).max() < 1e-6 and np.abs((one[1] - two[1] + 180) % 360 - 180).max() < 1e-6
    assert np.abs(one[0] - M.geolocate(tle, timing, y, x)[0]).max() > 1.0

    # two successive ascending equator crossings: 2 pi / (du/dt) apart, the longitudes by that time x (Earth's rate - dOmega/dt)
    def crossing(lo, hi):
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            if M.geolocate(tle, timing, [mid], [783.5])[0][0] < 0:
                lo = mid
            else:
                hi = mid
        return 0.5 * (lo + hi)
    per_line = timing.row_period / 8
    rev = 2 * np.pi / ref.orbit.u_dot / per_line
    first = crossing(-20.0 / 360 * rev, -10.0 / 360 * rev)                         # line 0 is 15 degrees past the node
    second = crossing(first + rev - 100, first + rev + 100)
    took = (second - first) * per_line
    lons = M.geolocate(tle, timing, [first, second], [783.5, 783.5])[1]
    want = -np.degrees(took * (R.EARTH_RATE - ref.orbit.raan_dot))
    print(f"nodal period {took:.6f} s (2 pi / du/dt = {2 * np.pi / ref.orbit.u_dot:.6f}); the node moves {lons[1] - lons[0]:.6f} degrees, expected {want:.6f}")
    assert abs(took - 2 * np.pi / ref.orbit.u_dot) < 1e-6 and abs((lons[1] - lons[0] - want + 180) % 360 - 180) < 1e-6
    assert 6000 < took < 6150 and -26 < want < -25


# --------------------------------------------------------------------------------------------------------------- time fit
def test_time_fit():
    """s is a whole number of microseconds in every stamp, so a double holds s, and the differences of two, to about 1e-11 s:
    1e-9 s is "exactly"."""
    from meteor_demod_amd import _capi, map as M
    rng = np.random.default_rng(8)
    rows, s0 = 200, 40000.25
    place, info = MU.packets(rows, s0)
    t = M.fit_time(place, info)
    print(f"clean: period {t.row_period!r}, s0 {t.s0!r}, {t.rows_fit} rows, {t.placed} packets, {t.lines} lines")
    assert abs(t.row_period - MU.ROW_PERIOD) < 1e-9 and abs(t.s0 - s0) < 1e-9 and (t.rows_fit, t.placed, t.lines) == (rows, rows * 42, 8 * rows)
    keep = np.broadcast_to(rng.random((rows, 1, 1)) >= 0.3, (rows, 3, 14)).copy()
    keep[-1] = True
    keep[0, 0, :5] = False                                                         # and the first row's first packets
    t = M.fit_time(*MU.packets(rows, s0, keep=keep))
    print(f"30 % of the rows missing: period {t.row_period!r}, s0 {t.s0!r}, {t.rows_fit} rows")
    assert abs(t.row_period - MU.ROW_PERIOD) < 1e-9 and abs(t.s0 - s0) < 1e-9 and 100 < t.rows_fit < 170 and t.lines == 8 * rows
    bad = info.copy()
    hit = np.flatnonzero(rng.random(info.size) < 0.05)
    bad["ms"][hit], bad["us"][hit] = rng.integers(0, 86400000, hit.size), rng.integers(0, 1000, hit.size)
    bad["ms"][0] = 86000000                                                        # the first stamp too
    t = M.fit_time(place, bad)
    print(f"5 % garbage: period {t.row_period!r}, s0 {t.s0!r}")
    assert abs(t.row_period - MU.ROW_PERIOD) < 1e-9 and abs(t.s0 - s0) < 1e-9
    t = M.fit_time(*MU.packets(rows, 86400.0 - 100.5))                              # midnight after 82 rows
    print(f"over midnight: period {t.row_period!r}, s0 {t.s0!r}")
    assert abs(t.row_period - MU.ROW_PERIOD) < 1e-9 and abs(t.s0 - (86400.0 - 100.5)) < 1e-9
    t = M.fit_time(*MU.packets(1, s0))
    assert t.row_period == 8 / 6.5 and abs(t.s0 - s0) < 1e-9 and t.rows_fit == 1
    t = M.fit_time(*MU.packets(1, s0), row_period=1.5)
    assert t.row_period == 1.5
    with pytest.raises(_capi.MdemodError) as e:
        M.fit_time(place[place["channel"] < 0], info[place["channel"] < 0])
    assert "no placed packet" in e.value.detail


def test_auto_date_is_the_one_nearest_the_epoch():
    from meteor_demod_amd import map as M
    tle = M.parse_tle(MU.tle_text())                                               # the epoch: day 19822, 12 h
    for s0, want in ((54000.0, 19822), (10800.0 + 100.0, 19822), (10800.0 - 2000.0, 19823), (10800.0 + 43200.0 + 100.0, 19822), (3000.0, 19823), (86000.0, 19822)):
        t = M.fit_time(*MU.packets(20, s0))                                        # (3000 s onboard is 21 h 50 UTC of the day before)
        got = M.resolve_date(tle, t)
        mid = s0 + 80 * t.row_period / 8 - 10800.0
        print(f"s0 {s0}: date {got}, the middle line {((got - 19822) * 86400 + mid - 43200) / 3600:+.2f} h from the epoch")
        assert got == want and abs((got - 19822) * 86400 + mid - 43200) <= 43200
    assert M.resolve_date(tle, M.fit_time(*MU.packets(20, 54000.0), date="2024-04-01")) == 19814


# ------------------------------------------------------------------------------------------------------------------ nodes
def test_nodes_equal_the_numpy_inverse():
    """Every node against the numpy model's own inverse of the node's point: 1 unit of 1/256 pixel, half a unit of rounding and
    half for the two solvers.  Missing nodes are missing in both."""
    tle, timing, ref = _pass()
    g = _grid()
    a, b = np.meshgrid(16 * np.arange(g.nodes.shape[0]), 16 * np.arange(g.nodes.shape[1]), indexing="ij")
    y, x = ref.inverse(*_centres(g, a, b), lines=8 * ROWS)
    none = (g.nodes[..., 0] == MU.NO_NODE) & (g.nodes[..., 1] == MU.NO_NODE)
    both = ~none & np.isfinite(y)
    ex, ey = np.abs(g.nodes[..., 0][both] - 256 * x[both]), np.abs(g.nodes[..., 1][both] - 256 * y[both])
    print(f"{g.width} x {g.height} at {g.sx} x {g.sy:g} px/deg from {g.lat_top:.2f}, {g.lon_left:.2f}; {g.nodes.shape[0]} x {g.nodes.shape[1]} nodes, "
          f"{int(none.sum())} missing ({int(np.isnan(y).sum())} in numpy); worst difference {ex.max():.3f} in X, {ey.max():.3f} in Y (1/256 pixel)")
    assert g.width % 4 == 0 and g.nodes.shape == MU.nodes_shape(g.width, g.height) and g.sx == round(100 * np.cos(np.radians(g.lat_top - g.height / 200)))
    assert np.array_equal(none, np.isnan(y)) and 0 < none.sum() < none.size // 2
    assert ex.max() <= 1.0 and ey.max() <= 1.0
    # the box holds the swath and no more than a pixel's rounding: the corners of the picture lie inside
    lat, lon = ref.forward(np.array([0.0, 0.0, 8 * ROWS - 1.0, 8 * ROWS - 1.0]), np.array([0.0, 1567.0, 0.0, 1567.0]))
    i, j = (g.lat_top - lat) * g.sy, ((lon - g.lon_left + 180) % 360 - 180) * g.sx
    assert (i >= 0).all() and (i <= g.height).all() and (j >= 0).all() and (j <= g.width).all()


def test_pass_over_the_date_line_and_refusals():
    from meteor_demod_amd import _capi, map as M
    tle, timing, ref = _pass()
    mid = ref.forward(4 * ROWS, 783.5)[1]
    text = MU.with_raan(150.0 + 180.0 - mid)
    ref180 = MU.ref_pass(ROWS, text=text)
    print(f"the middle of the pass lies at longitude {float(ref180.forward(4 * ROWS, 783.5)[1]):.3f}")
    assert abs(abs(ref180.forward(4 * ROWS, 783.5)[1]) - 180) < 0.01
    g, plain = M.grid(text, timing, 8 * ROWS), _grid()
    print(f"{g.width} x {g.height} from longitude {g.lon_left:.2f}; the plain pass is {plain.width} x {plain.height}")
    assert abs(g.width - plain.width) <= 8 and g.height == plain.height and -180 <= g.lon_left < 180
    rng = np.random.default_rng(3)
    a, b = rng.integers(0, g.nodes.shape[0], 3000), rng.integers(0, g.nodes.shape[1], 3000)
    y, x = ref180.inverse(*_centres(g, 16 * a, 16 * b), lines=8 * ROWS)
    got = g.nodes[a, b]
    none = (got[:, 0] == MU.NO_NODE) & (got[:, 1] == MU.NO_NODE)
    assert np.array_equal(none, np.isnan(y)) and np.abs(got[~none, 0] - 256 * x[~none]).max() <= 1.0 and np.abs(got[~none, 1] - 256 * y[~none]).max() <= 1.0
    # connected: as many nodes as the plain pass has
    count = lambda n: int(((n[..., 0] != MU.NO_NODE) | (n[..., 1] != MU.NO_NODE)).sum())
    assert abs(count(g.nodes) - count(plain.nodes)) < 0.02 * count(plain.nodes)
    for word, fn in (("beyond 85", lambda: M.grid(tle, M.fit_time(*MU.packets(ROWS, MU.mid_latitude_s0(50.0))), 8 * ROWS)),
                     ("fits", lambda: M.grid(tle, timing, 8 * ROWS, px_per_deg=300)), ("1 .. 1000", lambda: M.grid(tle, timing, 8 * ROWS, px_per_deg=1001)),
                     ("8192", lambda: M.grid(tle, timing, 8 * 8193)), ("multiple of 8", lambda: M.grid(tle, timing, 12)),
                     ("scan side", lambda: M.grid(tle, timing, 8 * ROWS, side=0)), ("scan angle", lambda: M.grid(tle, timing, 8 * ROWS, scan_deg=140))):
        with pytest.raises(_capi.MdemodError) as e:
            fn()
        print(f"{word}: '{e.value.detail}'")
        assert e.value.code == _capi.MDEMOD_ERR_PARAM and word in e.value.detail
    with pytest.raises(_capi.MdemodError) as e:
        M.grid(tle, timing, 8 * ROWS, px_per_deg=300)
    fit = int(re.search(r"scale of (\d+) fits", e.value.detail).group(1))
    ok = M.grid(tle, timing, 8 * ROWS, px_per_deg=fit)
    print(f"at 300 px/deg refused, the scale named is {fit}: {ok.width} x {ok.height}")
    assert ok.width <= 8192 and ok.height <= 16384 and fit > 100


# Worst difference between the interpolated and the exact source coordinates, in source pixels, over the pixels of 320 cells that
# fall inside the picture (profiles/map.md): measured 0.0513 at 100 px/deg and 0.2040 at 50, both in X.  The bars are 1.5 times that:
# they cover other orbits of the same family.
GRID_COST_BAR = {100: 1.5 * 0.0513, 50: 1.5 * 0.2040}


@pytest.mark.parametrize("scale", [100, 50])
def test_what_the_16_pixel_grid_costs(scale):
    tle, timing, ref = _pass()
    g = _grid(scale)
    rng = np.random.default_rng(16)
    n = g.nodes.astype(np.int64)
    whole = ~((n[..., 0] == MU.NO_NODE) & (n[..., 1] == MU.NO_NODE))
    cells = np.argwhere(whole[:-1, :-1] & whole[1:, :-1] & whole[:-1, 1:] & whole[1:, 1:])
    cells = cells[rng.choice(len(cells), 320, replace=False)]
    p, q = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    a, b = cells[:, 0][:, None, None], cells[:, 1][:, None, None]
    w = [(16 - p) * (16 - q), p * (16 - q), (16 - p) * q, p * q]
    corner = [n[a, b], n[a + 1, b], n[a, b + 1], n[a + 1, b + 1]]
    X = (sum(w[k] * corner[k][..., 0] for k in range(4)) + 128) >> 8
    Y = (sum(w[k] * corner[k][..., 1] for k in range(4)) + 128) >> 8
    y, x = ref.inverse(*_centres(g, 16 * a + p, 16 * b + q), lines=8 * ROWS)
    inside = (X >= 0) & (X <= 1567 * 256) & (Y >= 0) & (Y <= (8 * ROWS - 1) * 256) & np.isfinite(y)
    worst = max(np.abs(X / 256 - x)[inside].max(), np.abs(Y / 256 - y)[inside].max())
    print(f"{scale} px/deg: {int(inside.sum())} pixels of 320 cells inside the picture, worst difference {worst:.4f} source pixel "
          f"(X {np.abs(X / 256 - x)[inside].max():.4f}, Y {np.abs(Y / 256 - y)[inside].max():.4f}), bar {GRID_COST_BAR[scale]:.4f}")
    assert inside.sum() > 20000 and worst <= GRID_COST_BAR[scale]


# ------------------------------------------------------------------------------------------------------------- the model
@functools.lru_cache(maxsize=None)
def _source(kind="mixed"):
    return PU.pixels(MU.SRC_ROWS, 31), PU.masks(kind, MU.SRC_ROWS, 4), PU.random_luts(2)


def test_model_warp_on_hand_made_grids():
    """The model against the vectorised numpy restatement of the header on every case of the GPU test's list, grey and colour."""
    from meteor_demod_amd import map as M
    for kind in ("mixed", "empty1"):
        images, filled, luts = _source(kind)
        for name, w, h, nodes in MU.warp_cases():
            for select in ((2, 1, 0), (1,), (0, 0, 2)):
                out, val = M.model_warp(images, filled, select, luts[: len(select)], nodes, w, h, valid=True)
                want, want_val = MU.warp_reference(images, filled, select, luts, nodes, w, h)
                assert np.array_equal(out, want) and np.array_equal(val, want_val), (kind, name, select)
                assert np.array_equal(M.model_warp(images, filled, select, luts[: len(select)], nodes, w, h), want)
            print(f"{kind}, {name}: {w} x {h}, {np.count_nonzero(val)} of {val.size} pixels valid")


def test_model_warp_known_answers():
    """Cases whose answer needs no model: the identity, half a pixel, the border of a missing strip."""
    from meteor_demod_amd import map as M
    images, _, _ = _source()
    full = [np.ones((MU.SRC_ROWS, 14), np.uint8)] * 3
    ident = np.arange(256, dtype=np.uint8)[None].repeat(3, 0)
    cases = {c[0]: c for c in MU.warp_cases()}
    _, w, h, nodes = cases["identity"]
    out, val = M.model_warp(images, full, (0, 1, 2), ident, nodes, w, h, valid=True)
    assert np.array_equal(out, np.stack([im[:, 700:900] for im in images], -1)) and (val == 7).all()
    _, w, h, nodes = cases["identity, lines beyond the last"]
    out, val = M.model_warp(images, full, (1,), ident[:1], nodes, w, h, valid=True)
    assert np.array_equal(out[:24, :, 0], images[1][:, :36]) and not out[24:].any() and (val[:24] == 1).all() and not val[24:].any()
    _, w, h, nodes = cases["half a pixel"]
    out = M.model_warp(images, full, (2,), ident[:1], nodes, w, h)[:, :, 0]
    s = images[2].astype(np.int64)
    along = (s[:, 100:168] + s[:, 101:169] + 1) >> 1
    assert np.array_equal(out, ((along[:17] + along[1:18] + 1) >> 1).astype(np.uint8))
    # the border of a missing strip, across the columns (cell 6 | 7 at column 784) and across the lines (strip row 0 | 1 at line 8)
    mask = np.ones((MU.SRC_ROWS, 14), np.uint8)
    mask[1, 7], mask[2, 6] = 0, 0
    nodes = MU.affine_nodes(8, 24, lambda i, j: 256 * (j + 780) + 128, lambda i, j: 256 * i + 128)
    out, val = M.model_warp(images, [mask] * 3, (0,), ident[:1], nodes, 8, 24, valid=True)
    out, s = out[:, :, 0].astype(np.int64), images[0].astype(np.int64)
    mean = lambda a, b: (a + b + 1) >> 1
    assert out[2, 3] == mean(mean(s[2, 783], s[2, 784]), mean(s[3, 783], s[3, 784]))                      # all four taps filled
    assert out[9, 3] == mean(s[9, 783], s[10, 783]) and out[9, 4] == 0 and val[9, 4] == 0                  # the right taps missing; all missing
    assert out[7, 3] == mean(mean(s[7, 783], s[7, 784]), s[8, 783])                                        # the lower right tap missing
    assert out[7, 4] == mean(s[7, 784], s[7, 785]) and val[7, 4] == 1                                      # the lower line does not count
    assert out[15, 3] == mean(s[15, 783], s[16, 784]) and out[15, 2] == mean(s[15, 782], s[15, 783])       # one tap of each line; the lower line missing
    assert out[23, 4] == 0 and val[23, 4] == 0                                                             # half a line beyond the last line: empty


# ------------------------------------------------------------------------------------------------------------ end to end
SQUARE, E2E_ROWS = 1.0, 160


@functools.lru_cache(maxsize=None)
def e2e_case():
    """(pictures, masks, placements, reports, numpy pass, marked square): the scene through the numpy forward function, with holes."""
    rng = np.random.default_rng(21)
    ref = MU.ref_pass(E2E_ROWS)
    lat, lon = ref.forward(4 * E2E_ROWS, 600.0)
    marked = (float(np.floor(lat)), float(np.floor(lon)))
    keep = rng.random((E2E_ROWS, 3, 14)) >= 0.1
    place, info = MU.packets(E2E_ROWS, MU.mid_latitude_s0(), keep=keep)
    return MU.paint(ref, E2E_ROWS, SQUARE, marked), MU.filled_of(place, E2E_ROWS), place, info, ref, marked


def check_scene(m, marked, label):
    """Every valid pixel at least 3 output pixels from a square's edge has exactly its square's level; at least 60 % remain."""
    i, j = np.meshgrid(np.arange(m.height), np.arange(m.width), indexing="ij")
    lat, lon = m.lat_top - (i + 0.5) / m.sy, m.lon_left + (j + 0.5) / m.sx
    d_lat, d_lon = MU.edge_distance(lat, lon, SQUARE)
    far = (d_lat * m.sy >= 3.0) & (d_lon * m.sx >= 3.0)
    seen = 0
    for pl, ch in enumerate(m.select):
        ok = ((m.valid >> pl) & 1).astype(bool)
        want = MU.scene(lat, lon, ch, SQUARE, marked)
        wrong = ok & far & (m.pixels[..., pl] != want)
        share = (ok & far).sum() / max(ok.sum(), 1)
        print(f"{label}, plane {pl}: {int(ok.sum())} valid pixels, {100 * share:.1f} % kept, {int(wrong.sum())} wrong")
        assert not wrong.any() and share >= 0.6 and ok.sum() > 0.2 * ok.size
        seen += int((ok & far & (want == MU.MARKED_LEVEL)).sum())
    assert seen > 3 * 0.5 * (m.sy - 6) * (m.sx - 6)                                 # the marked square is there, at its own coordinates


def test_scene_through_the_cpu_model():
    from meteor_demod_amd import map as M
    images, filled, place, info, ref, marked = e2e_case()
    m = M.model_host(MU.tle_text(), images, filled, place, info, (2, 1, 0), stretch=0, px_per_deg=50, piece_lines=64)
    print(f"{m.width} x {m.height}, {100 * m.valid_share:.1f} % valid, marked square at {marked}")
    check_scene(m, marked, "model")
    whole = M.model_host(MU.tle_text(), images, filled, place, info, (2, 1, 0), stretch=0, px_per_deg=50, piece_lines=16384)
    assert np.array_equal(whole.pixels, m.pixels) and np.array_equal(whole.valid, m.valid)
    assert m.date == 19822 and m.rows_fit == E2E_ROWS and abs(m.row_period - MU.ROW_PERIOD) < 1e-9 and m.limits == [(0, 255)] * 3
    wld = [float(v) for v in m.world_file().split()]
    assert len(wld) == 6 and wld[0] == 1 / m.sx and wld[3] == -1 / m.sy and wld[1:3] == [0, 0] and wld[4] == m.lon_left + 0.5 / m.sx and wld[5] == m.lat_top - 0.5 / m.sy


# ---------------------------------------------------------------------------------------------------------------- binding
def _header_entries():
    return re.findall(r"^\s*(?:int|void|uint64_t)\s+(mdemod_\w+)\s*\(", (ROOT / "include" / "meteor_demod_amd_map.h").read_text(), re.M)


def test_map_entries_exported_and_bound():
    """Every entry of the new header is exported by the library and typed in map.py's own table; the older binding tables and
    headers are untouched; the model is exported beside them."""
    from meteor_demod_amd import _capi, image, map as M, picture
    names = _header_entries()
    assert sorted(names) == sorted(["mdemod_map_default_opts", "mdemod_map_parse_tle", "mdemod_map_fit_time", "mdemod_map_date", "mdemod_map_geolocate",
                                    "mdemod_map_grid", "mdemod_map_grid_free", "mdemod_map_warp_device", "mdemod_map_compose_host", "mdemod_map_free"])
    lib = M.lib()
    for n in names + list(M.MODEL_SIGNATURES):
        assert hasattr(lib, n), n
    assert sorted(M.SIGNATURES) == sorted(names)
    assert sorted(M.MODEL_SIGNATURES) == ["mdemod_map_model_host", "mdemod_map_model_warp"]
    others = list(_capi.SIGNATURES) + list(image.SIGNATURES) + list(image.MODEL_SIGNATURES) + list(picture.SIGNATURES) + list(picture.MODEL_SIGNATURES)
    assert not any("_map_" in n for n in others)
    for h in (ROOT / "include").glob("*.h"):
        if h.name != "meteor_demod_amd_map.h":
            assert "mdemod_map_" not in h.read_text(), h.name
    assert _capi.lib().mdemod_abi_version() == 5
    for f in ("parse_tle", "fit_time", "geolocate", "grid", "warp", "model_warp", "compose", "image_to_map", "model_host"):
        assert callable(getattr(M, f))


def test_map_int_entries_are_function_try_blocks():
    from meteor_demod_amd import map as M
    found = 0
    entries = set(_header_entries()) | set(M.MODEL_SIGNATURES)
    for src in (ROOT / "meteor_demod_amd" / "csrc" / "map.hip", ROOT / "meteor_demod_amd" / "csrc" / "map_host.cpp"):
        text = src.read_text()
        for m in re.finditer(r"^int\n(mdemod_\w+)\(", text, re.M):
            assert m.group(1) in entries, m.group(1)
            found += 1
            body = text[m.end():]
            assert body[: body.index("{")].rstrip().endswith("try"), f"{src.name}: {m.group(1)} is not a function-try-block"
            assert body[body.index("{"):].lstrip("{ ").startswith("MDEMOD_API_ENTER"), m.group(1)
            assert body[body.index("\n}"):].startswith("\n} MDEMOD_API_CATCH"), f"{src.name}: {m.group(1)} does not end in MDEMOD_API_CATCH"
    assert found == 2 + 7, found


def test_map_struct_layouts(tmp_path):
    import ctypes as C
    import subprocess
    from meteor_demod_amd import map as M
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "meteor_demod_amd_map.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", '
           'sizeof(mdemod_map_tle), sizeof(mdemod_map_opts), sizeof(mdemod_map_timing), sizeof(mdemod_map_nodes), sizeof(mdemod_map_result), '
           'offsetof(mdemod_map_tle, mean_motion), offsetof(mdemod_map_opts, piece_lines), offsetof(mdemod_map_timing, lines), offsetof(mdemod_map_nodes, nodes), '
           'offsetof(mdemod_map_result, utc0), offsetof(mdemod_map_result, valid)); return 0;}')
    (tmp_path / "s.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")], check=True)
    out = [int(x) for x in subprocess.run([str(tmp_path / "s")], capture_output=True, text=True, check=True).stdout.split()]
    print(out)
    assert out == [C.sizeof(M.MdemodMapTle), C.sizeof(M.MdemodMapOpts), C.sizeof(M.MdemodMapTiming), C.sizeof(M.MdemodMapNodes), C.sizeof(M.MdemodMapResult),
                   M.MdemodMapTle.mean_motion.offset, M.MdemodMapOpts.piece_lines.offset, M.MdemodMapTiming.lines.offset, M.MdemodMapNodes.nodes.offset,
                   M.MdemodMapResult.utc0.offset, M.MdemodMapResult.valid.offset]
    assert M.PLACEMENT.itemsize == 16 and M.STRIP_INFO.itemsize == 16


# ---------------------------------------------------------------------------------------------------- the C host, no map
def test_cli_without_map_layer_links_and_refuses(tmp_path):
    """The C host against tests/sanitize/stub_backend.c (which has no map layer): it links, --help lists --map and its options, and
    --map exits with status 1 saying what the library lacks - not "unrecognized option" - and writes nothing.  Against the real
    library --map without --image, an unreadable element set and a scale out of range are refused before anything is demodulated."""
    import subprocess
    import frames_util as U
    exe = tmp_path / "cli_stub"
    r = subprocess.run(["gcc", "-std=gnu11", "-O1", "-Wall", "-I", str(ROOT / "include"), str(ROOT / "host" / "meteor_demod_amd.c"),
                        str(ROOT / "tests" / "sanitize" / "stub_backend.c"), "-pthread", "-lm", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    h = subprocess.run([str(exe), "--help"], capture_output=True, text=True)
    assert h.returncode == 0 and all(w in h.stderr for w in ("--map <tle file>", "--norad", "--map-scale", "--date", "--time-offset", "--scan-side"))
    wav = tmp_path / "in.wav"
    wav.write_bytes(U.wav_bytes(288000, np.zeros((16384, 2), dtype=np.int16)))
    tle = MU.GOLDEN / "map_tle.txt"
    r = subprocess.run([str(exe), "-q", "-o", str(tmp_path / "out.s"), "--image", "--map", str(tle), str(wav)], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 1 and "no map layer" in r.stderr and "unrecognized" not in r.stderr, r.stderr
    assert r.stdout == "" and sorted(p.name for p in tmp_path.iterdir()) == ["cli_stub", "in.wav"]
    cli_exe = ROOT / "meteor_demod_amd" / "lib" / "meteor_demod_amd"
    for flags, word in ((("--map", str(tle)), "only with --image"), (("--image", "--map", str(tmp_path / "none.txt")), "could not read"),
                        (("--image", "--map", str(tle), "--map-scale", "1001"), "1 .. 1000"), (("--image", "--map", str(tle), "--norad", "5"), "catalogue number 5")):
        r = subprocess.run([str(cli_exe), "-q", "-o", str(tmp_path / "out.s"), *flags, str(wav)], capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == 1 and word in r.stderr and r.stdout == "", (flags, r.stderr)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["cli_stub", "in.wav"]
