"""CPU tests of the overlay layer (include/meteor_demod_amd_overlay.h): the host model against the independent Python model of
overlay_ref.py on 40 seeded pictures, the hand cases of the header's rule by value, the properties of the rule (opacity 0, order,
inside_only), the bins (the model through the tiles equals the model over every piece; the reach trap), the culling, the projection
against numpy, the graticule, both readers with every refusal, the binding and the C host without the layer.  No GPU."""
from __future__ import annotations

import math
import re
import struct
import subprocess

import numpy as np
import pytest

import overlay_ref as R
from conftest import GOLDEN, ROOT

TOP = 1 << 30


def _points(O, lines):
    xs = [np.asarray(a, dtype=np.int64) for a, _ in lines]
    first = np.concatenate([[0], np.cumsum([len(a) for a in xs])]).astype(np.uint32)
    return O.Points(np.concatenate(xs).astype(np.int32), np.concatenate([np.asarray(b, dtype=np.int64) for _, b in lines]).astype(np.int32), first)


def _ref_styles(styles):
    return [(s.half_width, s.opacity, s.colour, s.inside_only) for s in styles]


def random_case(seed):
    """A seeded picture with its styles and the polylines of each style: near the picture, zero-length segments, segments wholly
    outside, a segment of 10^6 pixels across the picture, vertices beyond 2^30."""
    from meteor_demod_amd import overlay as O
    rng = np.random.default_rng(1000 + seed)
    sizes = [(4, 1), (132, 70), (8, 5), (36, 33), (64, 32), (100, 36)]
    w, h = sizes[seed] if seed < len(sizes) else (4 * int(rng.integers(1, 34)), int(rng.integers(1, 71)))
    planes = 3 if seed % 2 else 1
    n_styles = 1 + seed % 4
    styles = [O.Style(int(rng.choice([0, 64, 128, 128, 300, 700, 2048])), int(rng.choice([256, 256, 160, 77, 0, 1])), tuple(int(v) for v in rng.integers(0, 256, 3)),
                      bool(rng.integers(0, 4) == 0)) for _ in range(n_styles)]
    lines = []
    for s in range(n_styles):
        mine = []
        for _ in range(int(rng.integers(1, 4))):
            n = int(rng.integers(2, 7))
            xs = rng.integers(-2000, 256 * w + 2000, n).astype(np.int64)
            ys = rng.integers(-2000, 256 * h + 2000, n).astype(np.int64)
            kind = int(rng.integers(0, 6))
            if kind == 0:                                   # a zero-length segment
                xs[1], ys[1] = xs[0], ys[0]
            elif kind == 1:                                 # wholly outside
                xs += 10_000_000
            elif kind == 2:                                 # 10^6 pixels, crossing the picture
                xs[0], xs[1] = 128 * w - 128_000_000, 128 * w + 128_000_000
                ys[0], ys[1] = 128 * h - int(rng.integers(0, 3000)), 128 * h + int(rng.integers(0, 3000))
            elif kind == 3:                                 # a vertex beyond 2^30 breaks the polyline
                xs[n // 2] = int(rng.choice([TOP + 1, -TOP - 1, 2**31 - 1, -2**31 + 1]))
            elif kind == 4:                                 # exactly 2^30 is still a vertex
                ys[0] = int(rng.choice([TOP, -TOP]))
            mine.append((xs, ys))
        lines.append(mine)
    pixels = rng.integers(0, 256, (h, w, 3) if planes == 3 else (h, w), dtype=np.uint8)
    valid = (rng.integers(0, 3, (h, w)) != 0).astype(np.uint8) * rng.integers(1, 256, (h, w)).astype(np.uint8)
    return w, h, styles, lines, pixels, valid


def case_pieces(O, w, h, styles, lines):
    parts = [O.pieces(_points(O, mine), s, styles[s].half_width, w, h) for s, mine in enumerate(lines)]
    return np.concatenate(parts)


# -------------------------------------------------------------------------------------------- model against the reference
def test_model_equals_the_python_reference():
    from meteor_demod_amd import overlay as O
    kept = made = 0
    for seed in range(40):
        w, h, styles, lines, pixels, valid = random_case(seed)
        pcs = case_pieces(O, w, h, styles, lines)
        ref_pieces = [p for s, mine in enumerate(lines) for xs, ys in mine for p in R.cut(xs, ys, s)]
        want, want_mask = R.draw(ref_pieces, _ref_styles(styles), pixels, valid)
        got, got_mask = O.model_pieces(pixels, pcs, styles, valid)
        tile_first, items = O.bins(pcs, styles, w, h)
        tiled, tiled_mask = O.model_tiles(pixels, pcs, tile_first, items, styles, valid)
        bad = int((got != want).sum()) + int((got_mask != want_mask).sum()) + int((tiled != want).sum()) + int((tiled_mask != want_mask).sum())
        kept += len(pcs)
        made += len(ref_pieces)
        # every piece the library kept is one of the reference's, record for record
        theirs = {(p[0], p[1], p[4], p[5], p[6], p[7]) for p in ref_pieces}
        assert all((int(p["ax"]), int(p["ay"]), int(p["tx"]), int(p["ty"]), int(p["L"]), int(p["style"])) in theirs for p in pcs), seed
        print(f"seed {seed}: {w} x {h} x {pixels.shape[2:] or 1}, {len(styles)} styles, {len(pcs)} of {len(ref_pieces)} pieces, {int((want_mask != 0).sum())} pixels drawn, {bad} bytes differ")
        assert bad == 0, seed
    assert made > 20 * kept > 0                              # the long segments are culled, and something is drawn


def test_hand_cases_of_the_rule():
    """A 1-pixel line on a pixel row gives 256 there and 0 beside it; half a pixel lower 128 and 128; a 45 degree line 256 on the
    diagonal and 75 beside it; the tangent's norm is within 0.11 % of 1 for pieces of at least 1/16 pixel."""
    from meteor_demod_amd import overlay as O
    zero = np.zeros((8, 8), dtype=np.uint8)
    black, white = [O.Style(128, 256, (255, 255, 255))], [O.Style(128, 256, (0, 0, 0))]
    on_black = np.array([(255 * a + 128) >> 8 for a in range(257)])
    on_white = np.array([(255 * (256 - a) + 128) >> 8 for a in range(257)])

    def alpha(lines):
        """The coverage a of every pixel: the one value that gives both the byte of a white line on black and of a black line on
        white."""
        pcs = O.pieces(_points(O, lines), 0, 128, 8, 8)
        up, down = O.model_pieces(zero, pcs, black)[0], O.model_pieces(zero + 255, pcs, white)[0]
        fits = (on_black[None, None, :] == up[..., None]) & (on_white[None, None, :] == down[..., None])
        assert (fits.sum(axis=2) == 1).all()
        return fits.argmax(axis=2)
    out = alpha([([-1000, 3000], [768, 768])])
    assert (out[3] == 256).all() and (out[2] == 0).all() and (out[4] == 0).all()
    out = alpha([([-1000, 3000], [896, 896])])
    assert (out[3] == 128).all() and (out[4] == 128).all() and (out[2] == 0).all() and (out[5] == 0).all()
    out = alpha([([0, 1792], [0, 1792])])
    assert [int(out[k, k]) for k in range(8)] == [256] * 8 and [int(out[k, k + 1]) for k in range(7)] == [75] * 7 and [int(out[k + 1, k]) for k in range(7)] == [75] * 7
    assert int(out[0, 2]) == 0
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(2000):
        dx, dy = (int(v) for v in rng.integers(-16384, 16385, 2))
        if dx * dx + dy * dy < 256:
            continue
        p = O.pieces(_points(O, [([100, 100 + dx], [100, 100 + dy])]), 0, 2048, 64, 64)
        if len(p):
            worst = max(worst, abs(math.hypot(int(p[0]["tx"]), int(p[0]["ty"])) / 16384 - 1))
    print(f"the tangent's norm is within {100 * worst:.4f} % of 1")
    assert worst < 0.0011


def test_properties_of_the_rule():
    """Opacity 0 leaves every byte; the order of the pieces does not matter; inside_only is honoured."""
    from meteor_demod_amd import overlay as O
    w, h, styles, lines, pixels, valid = random_case(1)
    pcs = case_pieces(O, w, h, styles, lines)
    assert len(pcs) > 10
    clear = [O.Style(s.half_width, 0, s.colour, s.inside_only) for s in styles]
    out, mask = O.model_pieces(pixels, pcs, clear, valid)
    assert np.array_equal(out, pixels) and mask.any()
    want = O.model_pieces(pixels, pcs, styles, valid)
    rng = np.random.default_rng(3)
    for _ in range(3):
        other = pcs[rng.permutation(len(pcs))]
        got = O.model_pieces(pixels, other, styles, valid)
        tf, it = O.bins(other, styles, w, h)
        tiled = O.model_tiles(pixels, other, tf, it, styles, valid)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)) and all(np.array_equal(a, b) for a, b in zip(tiled, want))
    inside = [O.Style(300, 256, (9, 200, 31), True)]
    line = O.pieces(_points(O, [([-500, 256 * w + 500], [128 * h, 128 * h + 700])]), 0, 300, w, h)
    free, free_mask = O.model_pieces(pixels, line, [O.Style(300, 256, (9, 200, 31), False)])
    out, mask = O.model_pieces(pixels, line, inside, valid)
    assert free_mask.any() and (valid[free_mask != 0] == 0).any() and (valid[free_mask != 0] != 0).any()
    assert np.array_equal(mask, np.where(valid != 0, free_mask, 0)) and np.array_equal(out, np.where((valid != 0)[..., None], free, pixels))
    with pytest.raises(Exception) as e:
        O.model_pieces(pixels, line, inside)
    assert "valid is needed" in str(e.value)


def test_bins_take_the_corner_of_the_cap():
    """The reach trap: the square cap of a 45 degree piece has a corner (w + 128) sqrt 2 from the end point along an axis.  A piece
    of the widest style ends 2600 units left of a tile, farther than w + 128 = 2176, in one of the tile's rows: it colours pixels of
    that tile, and the bins list it there."""
    from meteor_demod_amd import overlay as O
    w, h, half = 96, 96, 2048
    st = [O.Style(half, 256, (255, 0, 0))]
    end_x, end_y = 256 * 32 - 2600, 256 * 40                  # tile (1, 1) begins at pixel 32
    xs, ys = [end_x - 4000, end_x], [end_y - 4000, end_y]
    pcs = O.pieces(_points(O, [(xs, ys)]), 0, half, w, h)
    pixels = np.full((h, w, 3), 17, dtype=np.uint8)
    want, want_mask = O.model_pieces(pixels, pcs, st)
    tf, it = O.bins(pcs, st, w, h)
    got, got_mask = O.model_tiles(pixels, pcs, tf, it, st)
    print(f"the end point is {256 * 32 - end_x} units from the tile (w + 128 = {half + 128}); {int(want_mask[32:64, 32:64].sum())} pixels of tile (1, 1) drawn")
    assert 256 * 32 - end_x > half + 128 and want_mask[32:64, 32:64].any() and tf[4 + 1] > tf[4]
    assert np.array_equal(got, want) and np.array_equal(got_mask, want_mask)
    ref = R.draw(R.cut(xs, ys, 0), _ref_styles(st), pixels)
    assert np.array_equal(ref[0], want) and np.array_equal(ref[1], want_mask)


def test_culling_of_a_long_segment():
    """A segment of 10^6 pixels yields fewer pieces than the ceiling of its part inside the grown picture, plus 2."""
    from meteor_demod_amd import overlay as O
    for w, h, half, (x0, y0, x1, y1) in ((132, 70, 128, (-128_000_000, 5000, 128_000_000, 9000)), (64, 64, 2048, (3000, -128_000_000, 9000, 128_000_000)),
                                         (256, 256, 700, (-100_000_000, -100_000_000, 156_000_000, 156_000_000)), (64, 64, 128, (-128_000_000, 900_000, 128_000_000, 900_001))):
        pcs = O.pieces(_points(O, [([x0, x1], [y0, y1])]), 0, half, w, h)
        k = -(-max(abs(x1 - x0), abs(y1 - y0)) // 16384)
        reach = math.isqrt(2 * (half + 130) ** 2) + 2 + 2
        # the part of the segment inside the picture grown by the reach, in pieces
        t0, t1 = 0.0, 1.0
        for a, d, lo, hi in ((x0, x1 - x0, -reach, 256 * (w - 1) + reach), (y0, y1 - y0, -reach, 256 * (h - 1) + reach)):
            if d:
                ta, tb = sorted(((lo - a) / d, (hi - a) / d))
                t0, t1 = max(t0, ta), min(t1, tb)
            elif not lo <= a <= hi:
                t1 = -1.0
        inside = max(0.0, t1 - t0) * k
        print(f"{w} x {h}, half width {half}: {len(pcs)} pieces of {k}; {inside:.2f} pieces long inside the grown picture")
        assert len(pcs) < math.ceil(inside) + 2 and (len(pcs) > 0) == (inside > 0)
        whole = R.cut([x0, x1], [y0, y1], 0)
        assert len(whole) == k


# -------------------------------------------------------------------------------------------------------------- projection
def _np_project(g, lon, lat):
    wrap = lambda a: a - 360.0 * np.floor((a + 180.0) / 360.0)
    c = g.width / (2.0 * g.sx)
    dl = c + wrap(lon[0] - g.lon_left - c) + np.concatenate([[0.0], np.cumsum(wrap(np.diff(lon)))])
    return np.floor(256.0 * (dl * g.sx - 0.5) + 0.5), np.floor(256.0 * ((g.lat_top - lat) * g.sy - 0.5) + 0.5)


def test_projection_against_numpy():
    from meteor_demod_amd import overlay as O
    rng = np.random.default_rng(11)
    worst = 0
    for k in range(30):
        g = O.Geo(4 * int(rng.integers(8, 500)), int(rng.integers(8, 800)), int(rng.integers(1, 60)), float(rng.uniform(1, 100)), float(rng.uniform(-60, 80)),
                  float(rng.uniform(-180, 180)))
        n = int(rng.integers(2, 40))
        lon = g.lon_left + g.width / g.sx * rng.uniform(0.1, 0.9) + np.cumsum(rng.uniform(-0.5, 0.5, n))
        lon = lon - 360.0 * np.floor((lon + 180.0) / 360.0)
        lat = np.clip(g.lat_top - g.height / g.sy * rng.uniform(0.1, 0.9) + np.cumsum(rng.uniform(-0.5, 0.5, n)), -90, 90)
        p = O.project(g, O.vectors([(lon, lat)]))
        x, y = _np_project(g, lon, lat)
        assert len(p.first) >= 2
        # the copy at shift 0 is among what comes back; copies stand 92160 sx apart
        lines = [(p.x[a:b].astype(np.int64), p.y[a:b].astype(np.int64)) for a, b in zip(p.first[:-1], p.first[1:])]
        best = min(int(np.abs(px - x).max()) + int(np.abs(py - y).max()) for px, py in lines)
        worst = max(worst, best)
        for px, py in lines:
            shift = (px[0] - x[0]) / (92160 * g.sx)
            assert abs(shift - round(shift)) < 1e-4 and round(shift) in (-1, 0, 1)
    print(f"the fixed-point vertices are within {worst} units of numpy's")
    assert worst <= 1


def test_projection_is_continuous_across_the_date_line_and_gives_three_shifts():
    from meteor_demod_amd import overlay as O
    g = O.Geo(400, 100, 10, 10.0, 5.0, 160.0)                 # 160 E .. 200 E = 160 W
    v = O.vectors([([175.0, 179.5, -179.5, -175.0], [0.0, -1.0, -2.0, -3.0])])
    p = O.project(g, v)
    assert len(p.first) == 2
    x = p.x.astype(np.int64)
    assert list(x) == [256 * 150 - 128, 256 * 195 - 128, 256 * 205 - 128, 256 * 250 - 128] and list(p.y) == [256 * 50 - 128, 256 * 60 - 128, 256 * 70 - 128, 256 * 80 - 128]
    pcs = O.pieces(p, 0, 128, 400, 100)
    assert len(pcs) == 3 and all(int(q["L"]) < 16384 for q in pcs)                 # no piece runs the long way round
    # a map of the whole globe: a line on its left edge is also a line on its right edge
    world = O.Geo(720, 360, 2, 2.0, 90.0, -180.0)
    edge = O.project(world, O.vectors([([-180.0, -180.0], [10.0, -10.0])]))
    assert len(edge.first) == 3 and sorted(int(edge.x[a]) for a in edge.first[:-1]) == [-128, 256 * 720 - 128]
    far = O.project(world, O.vectors([([0.0, 0.0], [10.0, -10.0])]))
    assert len(far.first) == 2 and int(far.x[0]) == 256 * 360 - 128
    # a narrow map sees a line only once, whichever turn its longitudes are written in
    for lon in (170.0, -190.0):
        one = O.project(g, O.vectors([([lon, lon], [0.0, -5.0])]))
        assert len(one.first) == 2 and int(one.x[0]) == 256 * 100 - 128
    out = O.project(g, O.vectors([([0.0, 1.0], [0.0, -5.0])]))
    assert len(out.first) == 1 and out.x.size == 0
    with pytest.raises(Exception) as e:
        O.project(g, O.vectors([([0.0, float("nan")], [0.0, 1.0])]))
    assert "not a place" in str(e.value)


def test_graticule():
    """Rows and columns sit where lat_top, lon_left, sx and sy put them; auto picks the stated step."""
    from meteor_demod_amd import overlay as O
    g = O.Geo(240, 160, 8, 8.0, 62.0, 3.0)                    # 3 E .. 33 E, 62 N .. 42 N
    v = O.graticule(g, 5)
    meridians = sorted(float(a[0]) for a, b in v.lines() if len(a) == 2 and a[0] == a[1])
    parallels = sorted(float(b[0]) for a, b in v.lines() if (b == b[0]).all() and not (len(a) == 2 and a[0] == a[1]))
    assert meridians == [5, 10, 15, 20, 25, 30] and parallels == [45, 50, 55, 60]
    st = [O.Style(128, 256, (255, 255, 255)), O.Style(128, 256, (255, 255, 255))]
    out, mask = O.model_draw(np.zeros((160, 240), dtype=np.uint8), g, [(v, 1)], st, mask=True)
    assert set(np.unique(mask)) == {0, 2}
    # meridian 10 E stands at x = (10 - 3) 8 = 56: between the centres of columns 55 and 56; parallel 60 N at y = 16
    cols = np.flatnonzero(out[3] == 128)
    rows = np.flatnonzero(out[:, 3] == 128)
    assert list(cols) == [k for m in meridians for k in (int((m - 3) * 8) - 1, int((m - 3) * 8))], cols
    assert list(rows) == [k for p in reversed(parallels) for k in (int((62 - p) * 8) - 1, int((62 - p) * 8))], rows
    for sy, step in ((200.0, 1), (128.0, 1), (127.0, 2), (64.0, 2), (30.0, 5), (12.8, 10), (12.0, 15), (5.0, 30), (1.0, 30)):
        wide = O.Geo(64, 64, 1, sy, 80.0, 0.0)
        lats = sorted({float(b[0]) for a, b in O.graticule(wide, "auto").lines() if (b == b[0]).all() and len(b) > 1 and not (a == a[0]).all()} |
                      {float(b[0]) for a, b in O.graticule(O.Geo(64, int(61 * sy), 1, sy, 80.0, 0.0), 0).lines() if (b == b[0]).all() and not (a == a[0]).all()})
        assert len(lats) >= 2 and min(np.diff(lats)) == step, (sy, step, lats)
    # a map of the whole globe: parallels run the whole width, across +-180
    world = O.Geo(720, 360, 2, 2.0, 90.0, -180.0)
    out = O.model_draw(np.zeros((360, 720), dtype=np.uint8), world, [(O.graticule(world, 30), 0)], st)
    assert (out[59] == 128).all() and (out[60] == 128).all() and (out[100, ::60] == 128).all() and (out[100, 59::60] == 128).all() and int((out[100] != 0).sum()) == 24
    with pytest.raises(Exception) as e:
        O.graticule(g, 0.001)
    assert "step" in str(e.value)


# ----------------------------------------------------------------------------------------------------------------- readers
def _shp(records, code=9994, version=1000, length=None, tail=b""):
    body = b""
    for n, content in enumerate(records, 1):
        body += struct.pack(">ii", n, len(content) // 2) + content
    body += tail
    total = 100 + len(body) if length is None else length
    return struct.pack(">i5ii", code, 0, 0, 0, 0, 0, total // 2) + struct.pack("<ii8d", version, 3, 0, 0, 0, 0, 0, 0, 0, 0) + body


def _poly(kind, parts, points, extra=b""):
    return struct.pack("<i4dii", kind, 0, 0, 0, 0, len(parts), len(points)) + struct.pack(f"<{len(parts)}i", *parts) + b"".join(struct.pack("<2d", *p) for p in points) + extra


def test_readers(tmp_path):
    from meteor_demod_amd import _capi, overlay as O
    pts = [(10.0, 50.0), (11.0, 51.0), (12.0, 50.5), (-170.0, -5.0), (-171.0, -6.0)]
    recs = [_poly(3, [0], pts[:3]), struct.pack("<i", 0), _poly(5, [0, 3], pts), struct.pack("<i2d", 1, 3.0, 4.0),
            _poly(15, [0, 2], pts[:4], struct.pack("<2d4d", 0, 1, 1, 2, 3, 4) + b"\0" * 48), _poly(3, [], [])]
    shp = tmp_path / "lines.shp"
    shp.write_bytes(_shp(recs))
    v = O.read_vectors(shp)
    assert v.skipped == 2 and list(v.first) == [0, 3, 6, 8, 10, 12]
    assert list(v.lon) == [10, 11, 12, 10, 11, 12, -170, -171, 10, 11, 12, -170] and list(v.lat[:3]) == [50, 51, 50.5]
    # trailing bytes behind the header's length are not looked at
    (tmp_path / "tail.shp").write_bytes(_shp(recs[:1]) + b"\xff" * 7)
    assert O.read_vectors(tmp_path / "tail.shp").n_lines == 1
    text = tmp_path / "coast.txt"
    text.write_text("# a coast\n10 50\n11,51\n12\t50.5   # the cape\n\n-170 -5\r\n-171, -6\n>\n> another\n1e1 -9e1\n 20 5 \n# only a comment: ends nothing\n21 6\n")
    t = O.read_vectors(text)
    assert list(t.first) == [0, 3, 5, 8] and list(t.lon) == [10, 11, 12, -170, -171, 10, 20, 21] and list(t.lat) == [50, 51, 50.5, -5, -6, -90, 5, 6] and t.skipped == 0
    (tmp_path / "empty.txt").write_text("")
    assert O.read_vectors(tmp_path / "empty.txt").n_lines == 0

    def refused(name, data, word):
        (tmp_path / name).write_bytes(data)
        with pytest.raises(_capi.MdemodError) as e:
            O.read_vectors(tmp_path / name)
        print(f"{name}: '{e.value.detail}'")
        assert e.value.code == _capi.MDEMOD_ERR_PARAM and word in e.value.detail, (name, e.value.detail)
    good = _shp(recs[:1])
    refused("code.shp", _shp(recs[:1], code=9995), "file code")
    refused("version.shp", _shp(recs[:1], version=999), "version")
    refused("short.shp", good[:60], "header")
    refused("cut.shp", good[:-8], "past the file")
    refused("long.shp", _shp(recs[:1], length=len(good) + 40), "past the file")
    refused("record.shp", _shp([]) [:24] + struct.pack(">i", (100 + 8 + 20) // 2) + _shp([])[28:100] + struct.pack(">ii", 1, 400) + b"\0" * 20, "past the file")
    refused("half.shp", _shp([], tail=b"\0\0\0\1"), "its header runs past the file")
    refused("counts.shp", _shp([_poly(3, [0], pts[:3])[:-16]]), "past its own content length")
    refused("many.shp", _shp([struct.pack("<i4dii", 3, 0, 0, 0, 0, 1, 0x7fffffff) + b"\0" * 40]), "past its own content length")
    refused("tiny.shp", _shp([struct.pack("<i4d", 5, 0, 0, 0, 0)]), "past its own content length")
    refused("parts.shp", _shp([_poly(5, [0, 2, 2], pts)]), "must ascend")
    refused("down.shp", _shp([_poly(5, [0, 3, 1], pts)]), "must ascend")
    refused("outside.shp", _shp([_poly(5, [0, 5], pts)]), "must ascend")
    refused("negative.shp", _shp([_poly(5, [-1], pts)]), "must ascend")
    refused("type.shp", _shp([struct.pack("<i", 7)]), "shape type 7")
    refused("nan.shp", _shp([_poly(3, [0], [(1.0, 2.0), (float("nan"), 3.0)])]), "not finite")
    refused("inf.shp", _shp([_poly(3, [0], [(1.0, float("inf"))])]), "not finite")
    refused("lat.shp", _shp([_poly(3, [0], [(1.0, 90.5)])]), "beyond 90")
    refused("lon.shp", _shp([_poly(3, [0], [(-360.5, 9.0)])]), "beyond 360")
    refused("word.txt", b"10 50\n11 north\n", "line 2: not two numbers")
    refused("one.txt", b"10\n", "line 1: not two numbers")
    refused("three.txt", b"10 20 30\n", "line 1: not two numbers")
    refused("glued.txt", b"10 20x\n", "not two numbers")
    refused("nan.txt", b"10 nan\n", "not finite")
    refused("lat.txt", b"10 50\n10 -90.01\n", "line 2: latitude")
    refused("lon.txt", b"361 50\n", "beyond 360")
    refused("nul.txt", b"10 5\n1\x000 5\n", "not two numbers")
    with pytest.raises(_capi.MdemodError) as e:
        O.read_vectors(tmp_path / "none.shp")
    assert "could not open" in e.value.detail


# ----------------------------------------------------------------------------------------------------------------- binding
def _header_entries():
    return re.findall(r"^\s*(?:int|void|uint64_t)\s+(mdemod_\w+)\s*\(", (ROOT / "include" / "meteor_demod_amd_overlay.h").read_text(), re.M)


def test_overlay_entries_exported_and_bound():
    from meteor_demod_amd import _capi, map as MP, mosaic as M, overlay as O
    names = _header_entries()
    assert sorted(names) == sorted(O.SIGNATURES) and len(names) == 11
    lib = O.lib()
    for n in names + list(O.MODEL_SIGNATURES):
        assert hasattr(lib, n), n
    assert sorted(O.MODEL_SIGNATURES) == ["mdemod_overlay_model_draw", "mdemod_overlay_model_host", "mdemod_overlay_model_tiles"]
    listed = (ROOT / "meteor_demod_amd" / "csrc" / "overlay_host.h").read_text()
    assert all(n in listed for n in O.MODEL_SIGNATURES)
    others = list(_capi.SIGNATURES) + list(MP.SIGNATURES) + list(MP.MODEL_SIGNATURES) + list(M.SIGNATURES) + list(M.MODEL_SIGNATURES)
    assert not any("overlay" in n for n in others)
    for h in (ROOT / "include").glob("*.h"):
        if h.name != "meteor_demod_amd_overlay.h":
            assert "mdemod_overlay_" not in h.read_text(), h.name
    assert _capi.lib().mdemod_abi_version() == 5
    for f in ("read_vectors", "graticule", "project", "pieces", "draw", "model_draw", "draw_map"):
        assert callable(getattr(O, f))
    found = 0
    for src in ("overlay.hip", "overlay_host.cpp"):
        text = (ROOT / "meteor_demod_amd" / "csrc" / src).read_text()
        for m in re.finditer(r"^int\n(mdemod_\w+)\(", text, re.M):
            body = text[m.end():]
            assert body[: body.index("{")].rstrip().endswith("try") and body[body.index("\n}"):].startswith("\n} MDEMOD_API_CATCH"), m.group(1)
            found += 1
    assert found == 7 + 3


def test_overlay_struct_layouts(tmp_path):
    import ctypes as C
    from meteor_demod_amd import overlay as O
    names = ("geo", "vectors", "points", "piece", "pieces", "style", "bins", "layer", "report")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "meteor_demod_amd_overlay.h"\nint main(void){printf("' + "%zu " * (len(names) + 4) + '\\n", ' +
           ", ".join(f"sizeof(mdemod_overlay_{n})" for n in names) + ", offsetof(mdemod_overlay_geo, sy), offsetof(mdemod_overlay_style, inside_only), "
           "offsetof(mdemod_overlay_bins, n_items), offsetof(mdemod_overlay_report, tiles)); return 0;}")
    (tmp_path / "s.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")], check=True)
    out = [int(x) for x in subprocess.run([str(tmp_path / "s")], capture_output=True, text=True, check=True).stdout.split()]
    print(out)
    assert out == [C.sizeof(O.MdemodOverlayGeo), C.sizeof(O.MdemodOverlayVectors), C.sizeof(O.MdemodOverlayPoints), O.PIECE.itemsize, C.sizeof(O.MdemodOverlayPieces),
                   C.sizeof(O.MdemodOverlayStyle), C.sizeof(O.MdemodOverlayBins), C.sizeof(O.MdemodOverlayLayer), C.sizeof(O.MdemodOverlayReport),
                   O.MdemodOverlayGeo.sy.offset, O.MdemodOverlayStyle.inside_only.offset, O.MdemodOverlayBins.n_items.offset, O.MdemodOverlayReport.tiles.offset]
    assert O.PIECE.itemsize == 32 and C.sizeof(O.MdemodOverlayStyle) == 12


def test_model_host_in_bands_and_its_report():
    """The whole-picture entry's model path in bands of 32 and 64 lines equals one batch; the report counts what was drawn; the
    arguments' refusals come with their texts."""
    from meteor_demod_amd import _capi, overlay as O
    g = O.Geo(100, 150, 6, 5.0, 40.0, -12.0)
    rng = np.random.default_rng(2)
    coast = O.vectors([(-12 + np.cumsum(rng.uniform(0, 1.5, 14)), 38 - np.cumsum(rng.uniform(0, 2.4, 14))), ([-5.0, 0.0, -5.0], [30.0, 20.0, 12.0])])
    layers, st = [(coast, 0), (O.graticule(g, 5), 1)], O.default_styles(width=2.5)
    st[1].inside_only = True
    pixels = rng.integers(0, 256, (150, 100, 3), dtype=np.uint8)
    valid = (rng.integers(0, 2, (150, 100)) * 7).astype(np.uint8)
    want, want_mask, rep = O._host(O.lib().mdemod_overlay_model_host, "model", pixels, g, layers, st, valid, True, 0, ())
    pcs = O.layer_pieces(g, layers, st)
    direct = O.model_pieces(pixels, pcs, st, valid)
    assert np.array_equal(direct[0], want) and np.array_equal(direct[1], want_mask) and (want != pixels).any()
    assert rep.pieces == [int((pcs["style"] == s).sum()) for s in range(2)] and rep.pixels == [int(((want_mask >> s) & 1).sum()) for s in range(2)]
    tf, it = O.bins(pcs, st, 100, 150)
    assert rep.tiles == int((np.diff(tf.astype(np.int64)) > 0).sum()) and rep.items == it.size and min(rep.pixels) > 0
    for piece in (32, 64):
        got, got_mask = O.model_draw(pixels, g, layers, st, valid, mask=True, piece_lines=piece)
        assert np.array_equal(got, want) and np.array_equal(got_mask, want_mask), piece
    grey = O.model_draw(pixels[:, :, 0], g, layers, st, valid)
    assert grey.shape == (150, 100) and (grey != pixels[:, :, 0]).any()
    for word, fn in (("piece_lines", lambda: O.model_draw(pixels, g, layers, st, valid, piece_lines=48)), ("valid is needed", lambda: O.model_draw(pixels, g, layers, st)),
                     ("style 2 of 2", lambda: O.model_draw(pixels, g, [(coast, 2)], st, valid)), ("styles (1 .. 4)", lambda: O.model_draw(pixels, g, layers, st * 3, valid)),
                     ("half width", lambda: O.model_draw(pixels, g, layers, [O.Style(2049)], valid)), ("opacity", lambda: O.model_draw(pixels, g, layers, [O.Style(1, 257)], valid)),
                     ("width of 102", lambda: O.model_draw(np.zeros((150, 102), np.uint8), O.Geo(102, 150, 6, 5.0, 40.0, -12.0), layers[:1], st[:1])),
                     ("scale", lambda: O.model_draw(pixels, O.Geo(100, 150, 0, 5.0, 40.0, -12.0), layers, st, valid))):
        with pytest.raises(_capi.MdemodError) as e:
            fn()
        print(f"{word}: '{e.value.detail}'")
        assert e.value.code == _capi.MDEMOD_ERR_PARAM and word in e.value.detail


# ------------------------------------------------------------------------------------------------- the C host, no overlay
def test_cli_without_overlay_layer_links_and_refuses(tmp_path):
    """The C host against tests/sanitize/stub_backend.c (which has no overlay layer): it links, --help lists the options, and
    --overlay / --graticule exit with status 1 saying what the library lacks, and write nothing.  Against the real library the
    options without --map, a fourth file, a bad colour, width or step and a refused vector file exit with 1 before anything is
    demodulated, the vector file with the library's text."""
    import frames_util as U
    exe = tmp_path / "cli_stub"
    r = subprocess.run(["gcc", "-std=gnu11", "-O1", "-Wall", "-I", str(ROOT / "include"), str(ROOT / "host" / "meteor_demod_amd.c"),
                        str(ROOT / "tests" / "sanitize" / "stub_backend.c"), "-pthread", "-lm", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    h = subprocess.run([str(exe), "--help"], capture_output=True, text=True)
    assert h.returncode == 0 and all(w in h.stderr for w in ("--overlay <file>", "--graticule <deg>", "--overlay-colour <rrggbb>", "--overlay-width <px>"))
    wav = tmp_path / "in.wav"
    wav.write_bytes(U.wav_bytes(288000, np.zeros((16384, 2), dtype=np.int16)))
    coast = tmp_path / "coast.txt"
    coast.write_text("10 50\n11 51\n")
    tle = GOLDEN / "map_tle.txt"
    for flags in (("--overlay", str(coast)), ("--graticule", "5")):
        r = subprocess.run([str(exe), "-q", "-o", str(tmp_path / "out.s"), "--image", "--map", str(tle), *flags, str(wav)], capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == 1 and "no overlay layer" in r.stderr and "unrecognized" not in r.stderr and r.stdout == "", r.stderr
    cli_exe = ROOT / "meteor_demod_amd" / "lib" / "meteor_demod_amd"
    bad = tmp_path / "bad.txt"
    bad.write_text("10 50\n11 95\n")
    m = ("--image", "--map", str(tle))
    for flags, word in ((("--overlay", str(coast)), "only with --map"), (("--image", "--graticule", "auto"), "only with --map"),
                        ((*m, "--overlay-colour", "ff0000"), "only with --overlay"), ((*m, "--overlay", str(coast), "--overlay-colour", "ff00"), "rrggbb"),
                        ((*m, "--overlay", str(coast), "--overlay-colour", "ff00zz"), "rrggbb"), ((*m, "--overlay", str(coast), "--overlay-width", "17"), "0 .. 16"),
                        ((*m, "--graticule", "0"), "auto"), ((*m, "--graticule", "five"), "auto"), ((*m, *(["--overlay", str(coast)] * 4)), "at most 3"),
                        ((*m, "--overlay", str(bad)), "line 2: latitude 95 is beyond 90"), ((*m, "--overlay", str(tmp_path / "none.shp")), "could not open")):
        r = subprocess.run([str(cli_exe), "-q", "-B", *flags, str(wav)], capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == 1 and word in r.stderr and r.stdout == "", (flags, r.stderr)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["bad.txt", "cli_stub", "coast.txt", "in.wav"]
